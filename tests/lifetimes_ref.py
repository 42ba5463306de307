"""The lifetime correlations of include/molar_hip.h (molar_hip_lifetimes) restated in dense numpy: the bool matrix, gap filling by
the p / q definition, and the sums as written.  Case builders from seeded on/off Markov chains and hand-made rows.  Everything
here is an integer: the tests compare for equality."""
import numpy as np


def dense(frame_offsets, row_of_entry, nrows):
    """h[r, t] = row r occurs among the entries of frame t"""
    off = np.asarray(frame_offsets, np.int64)
    rows = np.asarray(row_of_entry, np.int64)
    F = off.shape[0] - 1
    h = np.zeros((nrows, F), bool)
    for t in range(F):
        h[rows[off[t]:off[t + 1]], t] = True
    return h


def sparse(h, rng=None, duplicates=0):
    """(frame_offsets uint64 [F + 1], row_of_entry uint32 [E]) of a dense matrix; with rng the rows of a frame come in random
    order, and `duplicates` entries of every frame that has any are named once more."""
    R, F = h.shape
    off, rows = [0], []
    for t in range(F):
        r = np.nonzero(h[:, t])[0]
        if rng is not None:
            if duplicates and r.shape[0]:
                r = np.concatenate([r, rng.choice(r, duplicates)])
            r = rng.permutation(r)
        rows.append(r)
        off.append(off[-1] + r.shape[0])
    return np.asarray(off, np.uint64), (np.concatenate(rows) if rows else np.zeros(0)).astype(np.uint32)


def fill_gaps(h, gap):
    """h'[r, u] = h[r, u], or there are p < u < q with h[r, p] = h[r, q] = 1 and q - p - 1 <= gap"""
    R, F = h.shape
    out = h.copy()
    if gap <= 0:
        return out
    for r in range(R):
        on = np.nonzero(h[r])[0]
        for p, q in zip(on[:-1], on[1:]):          # consecutive present frames: the narrowest bracket of every u between them
            if q - p - 1 <= gap:
                out[r, p:q] = True
    return out


def count(F, max_lag, origin_stride):
    tau = np.arange(max_lag + 1, dtype=np.int64)
    return ((F - 1 - tau) // origin_stride + 1).astype(np.uint64)


def runs_of(row):
    """lengths of the maximal runs of a bool row, in order"""
    x = np.concatenate([[0], row.astype(np.int8), [0]])
    d = np.diff(x)
    return np.nonzero(d == -1)[0] - np.nonzero(d == 1)[0]


def reference(frame_offsets, row_of_entry, nrows, groups=None, ngroups=None, max_lag=None, origin_stride=1, gap=0):
    """dict(inter, cont [G, L + 1] uint64, run_hist [G, F + 1] uint64, events, longest, present [R] uint32, count [L + 1])"""
    h = fill_gaps(dense(frame_offsets, row_of_entry, nrows), gap)
    R, F = h.shape
    L = F - 1 if max_lag is None else max_lag
    g = np.zeros(R, np.int64) if groups is None else np.asarray(groups, np.int64)
    G = 1 if groups is None else int(ngroups)
    inter = np.zeros((G, L + 1), np.uint64)
    cont = np.zeros((G, L + 1), np.uint64)
    hist = np.zeros((G, F + 1), np.uint64)
    origins = np.arange(0, F, origin_stride)
    alive = h.copy()                                # alive[r, t] = prod_{u = t .. t + tau} h[r, u], for t + tau <= F - 1
    for tau in range(L + 1):
        t = origins[origins + tau <= F - 1]
        if tau:
            alive = alive[:, :-1] & h[:, tau:]
        pi = (h[:, t] & h[:, t + tau]).sum(axis=1)
        pc = alive[:, t].sum(axis=1)
        np.add.at(inter[:, tau], g, pi.astype(np.uint64))
        np.add.at(cont[:, tau], g, pc.astype(np.uint64))
    events = np.zeros(R, np.uint32)
    longest = np.zeros(R, np.uint32)
    for r in range(R):
        ls = runs_of(h[r])
        events[r] = ls.shape[0]
        longest[r] = ls.max() if ls.shape[0] else 0
        np.add.at(hist[g[r]], ls, np.uint64(1))
    return dict(inter=inter, cont=cont, run_hist=hist, events=events, longest=longest, present=h.sum(axis=1).astype(np.uint32),
                count=count(F, L, origin_stride), dense=h)


def literal(frame_offsets, row_of_entry, nrows, groups, ngroups, max_lag, origin_stride, gap):
    """the same by loops over single frames, for tiny inputs: nothing shared with reference() but the argument list"""
    off = [int(x) for x in frame_offsets]
    F = len(off) - 1
    h = [[0] * F for _ in range(nrows)]
    for t in range(F):
        for e in range(off[t], off[t + 1]):
            h[int(row_of_entry[e])][t] = 1
    hp = [row[:] for row in h]
    for r in range(nrows):
        for u in range(F):
            for p in range(u):
                for q in range(u + 1, F):
                    if h[r][p] and h[r][q] and q - p - 1 <= gap:
                        hp[r][u] = 1
    G = 1 if groups is None else ngroups
    inter = [[0] * (max_lag + 1) for _ in range(G)]
    cont = [[0] * (max_lag + 1) for _ in range(G)]
    hist = [[0] * (F + 1) for _ in range(G)]
    events, longest, present = [0] * nrows, [0] * nrows, [0] * nrows
    for r in range(nrows):
        g = 0 if groups is None else int(groups[r])
        for tau in range(max_lag + 1):
            t = 0
            while t + tau <= F - 1:
                inter[g][tau] += hp[r][t] * hp[r][t + tau]
                prod = 1
                for u in range(t, t + tau + 1):
                    prod *= hp[r][u]
                cont[g][tau] += prod
                t += origin_stride
        run = 0
        for u in range(F + 1):
            if u < F and hp[r][u]:
                run += 1
                present[r] += 1
            elif run:
                hist[g][run] += 1
                events[r] += 1
                longest[r] = max(longest[r], run)
                run = 0
    return dict(inter=np.asarray(inter, np.uint64), cont=np.asarray(cont, np.uint64), run_hist=np.asarray(hist, np.uint64),
                events=np.asarray(events, np.uint32), longest=np.asarray(longest, np.uint32), present=np.asarray(present, np.uint32))


# ---------------------------------------------------------------- cases

def markov(R, F, p_on, p_off, seed):
    """R independent on/off chains over F frames: off -> on with p_on, on -> off with p_off, started from the stationary state"""
    rng = np.random.default_rng(seed)
    h = np.zeros((R, F), bool)
    state = rng.random(R) < p_on / (p_on + p_off)
    for t in range(F):
        h[:, t] = state
        u = rng.random(R)
        state = np.where(state, u >= p_off, u < p_on)
    return h


def hand_rows(F):
    """The rows every size is tried with, as far as F allows: empty, full, a single bit at either end, a run across a word
    boundary, runs of exactly 64 and 65, two bits on either side of a word boundary, gaps of 1, 2, 63 and 64 frames."""
    rows = [np.zeros(F, bool), np.ones(F, bool)]

    def row(*spans):
        x = np.zeros(F, bool)
        for a, b in spans:
            if a < F:
                x[a:min(b, F)] = True
        return x

    rows += [row((0, 1)), row((F - 1, F)), row((60, 70)), row((1, 65)), row((3, 68)), row((0, 64)), row((64, 128)),
             row((63, 64), (64, 65)), row((63, 64), (65, 66)), row((62, 63), (65, 66)), row((0, 1), (64, 65)), row((0, 1), (65, 66)),
             row((5, 6), (70, 71), (72, 73), (75, 76)), row((127, 128), (128, 129)), row((120, 127), (129, 140), (255, 257)),
             row((0, 1), (F - 1, F))]
    return np.stack(rows)


def case(R, F, seed, p_on=0.2, p_off=0.3, duplicates=2, empty_frames=()):
    """R rows over F frames: the hand-made rows first (as many as fit), Markov chains behind them; frames come out in random
    row order with some entries named twice; `empty_frames` have no entry at all.  Returns (h, frame_offsets, row_of_entry)."""
    rng = np.random.default_rng(seed)
    h = markov(R, F, p_on, p_off, seed + 1)
    hand = hand_rows(F)[:R]
    h[:hand.shape[0]] = hand
    for t in empty_frames:
        if t < F:
            h[:, t] = False
    off, rows = sparse(h, rng, duplicates)
    return h, off, rows
