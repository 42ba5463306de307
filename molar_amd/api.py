"""Host-side mirror of the pymolar surface for the accelerated path, over the C ABI.

Mirrors (same names, argument meaning, error behaviour) the Python front-end of the reference
for this path — molar_python/python/pymolar/molar.pyi:130-213 and molar_python/src/lib.rs:
    distance_search(cutoff | "vdw", sel1, sel2=None, dims=None) -> (pairs[N,2], dist[N])
    fit_transform(sel1, sel2), fit_transform_at_origin, rmsd(sel1, sel2) [rmsd_py], rmsd_mw
    Sel.com(dims) / cog(dims) / gyration() / inertia() / min_max() / apply_transform / unwrap_simple
    PeriodicBox(vectors, angles) / PeriodicBox.from_matrix, shortest_vector, ...
Only the numeric path is here: no selection language, no file IO (out of scope).
Arrays may be numpy (host) or torch CUDA tensors (device-resident, used in place).
"""
from __future__ import annotations

import collections
import ctypes as C

import numpy as np

from . import _lib
from ._lib import (MEMBRANE_ARRAYS, Box, ContactGroups, MembraneDesc, MembraneOut, MembraneView, MolarHipError, SearchDesc, SearchDescF64,
                   check)

PBC_FULL = 7
PBC_NONE = 0

SEARCH_SINGLE, SEARCH_DOUBLE, SEARCH_WITHIN, SEARCH_DOUBLE_VDW = 0, 1, 2, 3

ERR_NO_SEARCH = 52                                 # MOLAR_HIP_ERR_NO_SEARCH
LIFETIME_OUTPUTS = ("inter", "cont", "run_hist", "events", "longest", "present")      # in the order of the C ABI


def _is_torch(x) -> bool:
    return type(x).__module__.startswith("torch")


def _addr(x):
    """(address, keepalive) of a numpy array or a torch tensor; None -> (None, None)."""
    if x is None:
        return None, None
    if _is_torch(x):
        assert x.is_contiguous()
        return x.data_ptr(), x
    return x.ctypes.data, x


class _DevicePointer:
    """__cuda_array_interface__ holder for memory the engine owns (result buffers of the resident search)."""

    def __init__(self, addr, count, typestr):
        self.__cuda_array_interface__ = {"shape": (count,), "typestr": typestr, "data": (int(addr), False), "version": 2}


def device_view(addr, shape, dtype):
    """A torch CUDA tensor over `addr` (no copy).  The memory stays owned by the engine: the view is valid until the
    next search on the same context (or result set, for the begin/end form) reuses the buffer."""
    import torch
    count = int(np.prod(shape))
    if count == 0:
        return torch.empty(shape, dtype=dtype, device="cuda")
    typestr = {torch.int32: "<i4", torch.float32: "<f4", torch.int64: "<i8", torch.uint8: "|u1"}[dtype]
    return torch.as_tensor(_DevicePointer(addr, count, typestr), device="cuda").view(*shape)


def _f32(x, shape=None):
    if x is None:
        return None
    if _is_torch(x):
        import torch
        assert x.dtype == torch.float32
        return x.contiguous()
    a = np.ascontiguousarray(x, dtype=np.float32)
    return a.reshape(shape) if shape is not None else a


def _u64(x):
    if x is None:
        return None
    if _is_torch(x):
        import torch
        if x.dtype == torch.int64:
            return x.contiguous()     # non-negative int64 has the same bits as uint64
        raise TypeError("index tensors must be int64")
    return np.ascontiguousarray(x, dtype=np.uint64)


def _u32(x):
    """Group labels: numpy uint32, or a torch int32 tensor (non-negative int32 has the same bits as uint32)."""
    if x is None:
        return None
    if _is_torch(x):
        import torch
        if x.dtype == torch.int32:
            return x.contiguous()
        raise TypeError("label tensors must be int32")
    return np.ascontiguousarray(x, dtype=np.uint32)


_NO_ATOMS = np.zeros(1, np.uint64)[:0]      # an empty selection with an address


def _sel(x):
    """A selection for a search descriptor.  There a NULL index means "all atoms", and an empty torch tensor has no address
    (data_ptr() == 0): an empty selection, device or host, is passed as an empty host array that has one."""
    x = _u64(x)
    if x is not None and x.shape[0] == 0:
        return _NO_ATOMS
    return x


def pbc_mask(dims) -> int:
    """PbcDims::new (periodic_box.rs:101-107); None -> all False like the Python front-end."""
    if dims is None:
        return 0
    if isinstance(dims, (int, np.integer)):
        return int(dims) & 7
    return (1 if dims[0] else 0) | (2 if dims[1] else 0) | (4 if dims[2] else 0)


class PeriodicBox:
    """periodic_box.rs:146-435 (host arithmetic of the engine, identical to its device code)."""

    def __init__(self, vectors=None, angles=None, _box=None):
        lib = _lib.load()
        self._b = Box()
        if _box is not None:
            self._b = _box
        else:
            v, a = vectors, angles
            check(lib.molar_hip_box_from_vectors_angles(v[0], v[1], v[2], a[0], a[1], a[2], C.byref(self._b)))

    @classmethod
    def from_matrix(cls, m):
        """m: 3x3 with COLUMNS = box vectors a,b,c (periodic_box.rs:7-13)."""
        lib = _lib.load()
        m = np.asarray(m, dtype=np.float32).reshape(3, 3)
        flat = np.ascontiguousarray(m.T).reshape(9)
        b = Box()
        check(lib.molar_hip_box_from_matrix(flat.ctypes.data, C.byref(b)))
        return cls(_box=b)

    def get_matrix(self):
        return np.array(self._b.m, dtype=np.float32).reshape(3, 3).T.copy()

    def colmajor9(self):
        return np.array(self._b.m, dtype=np.float32)

    def shortest_vector(self, v, dims=PBC_FULL):
        v = np.ascontiguousarray(v, dtype=np.float32)
        out = np.zeros(3, np.float32)
        _lib.load().molar_hip_box_shortest_vector(C.byref(self._b), v.ctypes.data, pbc_mask(dims), out.ctypes.data)
        return out

    def closest_image(self, point, target, dims=PBC_FULL):
        point = np.asarray(point, np.float32); target = np.asarray(target, np.float32)
        return target + self.shortest_vector(point - target, dims)

    def distance(self, p1, p2, dims=PBC_FULL):
        p1 = np.asarray(p1, np.float32); p2 = np.asarray(p2, np.float32)
        s = self.shortest_vector(p2 - p1, dims)
        return float(np.sqrt(np.float32(s[0] * s[0] + s[1] * s[1]) + np.float32(s[2] * s[2])))

    def get_lab_extents(self):
        out = np.zeros(3, np.float32)
        _lib.load().molar_hip_box_lab_extents(C.byref(self._b), out.ctypes.data)
        return out

    def _v3(self, fn, v):
        v = np.ascontiguousarray(v, dtype=np.float32)
        out = np.zeros(3, np.float32)
        getattr(_lib.load(), fn)(C.byref(self._b), v.ctypes.data, out.ctypes.data)
        return out

    def to_box_coords(self, v):
        return self._v3("molar_hip_box_to_box_coords", v)

    def to_lab_coords(self, v):
        return self._v3("molar_hip_box_to_lab_coords", v)

    def wrap_point(self, p):
        return self._v3("molar_hip_box_wrap_point", p)

    def is_inside(self, p):
        p = np.ascontiguousarray(p, dtype=np.float32)
        return bool(_lib.load().molar_hip_box_is_inside(C.byref(self._b), p.ctypes.data))

    def get_box_extents(self):
        out = np.zeros(3, np.float32)
        _lib.load().molar_hip_box_extents(C.byref(self._b), out.ctypes.data)
        return out

    def is_triclinic(self):
        m = self._b.m
        return any(m[k] != 0.0 for k in (1, 2, 3, 5, 6, 7))

    @property
    def n_tric_corrections(self):
        return int(self._b.nshift)


class Engine:
    """One molar_hip_ctx: a GPU, a stream and reusable device buffers.

    The context runs on a stream of its own unless `stream` is given (e.g. `torch.cuda.current_stream().cuda_stream`).
    Device tensors handed to it are read where they are, on THAT stream: a tensor another stream is still producing (a
    `.clone()`, a `torch.randn(...)` enqueued a moment ago) has to be complete first - `torch.cuda.synchronize()`, or one
    shared stream."""

    def __init__(self, device: int = 0, stream=None):
        self.lib = _lib.load()
        self.ctx = self.lib.molar_hip_create(device)
        if not self.ctx:
            raise MolarHipError(100, _lib.last_error())
        self.device = device
        if stream is not None:
            check(self.lib.molar_hip_set_stream(self.ctx, C.c_void_p(stream)))

    def close(self):
        if getattr(self, "ctx", None):
            for ref in list(getattr(self, "_plans", ())):        # plans hold the context: they go first
                plan = ref()
                if plan is not None:
                    plan.close()
            self.lib.molar_hip_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _adopt(self, plan):
        import weakref
        if not hasattr(self, "_plans"):
            self._plans = []
        self._plans = [r for r in self._plans if r() is not None] + [weakref.ref(plan)]

    def synchronize(self):
        check(self.lib.molar_hip_synchronize(self.ctx))

    PROFILE_CLASSES = ("grid_build", "pair_count", "offset_scan", "pair_fill", "measure", "search_frame")

    def profile_enable(self, on=True):
        """True / 1: a span per kernel class; 2: one span per resident search (class search_frame); False: off."""
        check(self.lib.molar_hip_profile_enable(self.ctx, int(on)))

    def profile_read(self):
        """{class: (milliseconds, launches)} accumulated since the last read (HIP events)."""
        ms = (C.c_float * 8)(); ln = (C.c_uint64 * 8)()
        check(self.lib.molar_hip_profile_read(self.ctx, ms, ln))
        return {name: (float(ms[k]), int(ln[k])) for k, name in enumerate(self.PROFILE_CLASSES)}

    # ------------------------------------------------------------ search
    def _search_desc(self, kind, cutoff, xyz1, idx1=None, xyz2=None, idx2=None, box=None, pbc=0, vdw1=None,
                     vdw2=None, ids_local=False, lower=None, upper=None):
        xyz1 = _f32(xyz1); xyz2 = _f32(xyz2); idx1 = _sel(idx1); idx2 = _sel(idx2)
        vdw1 = _f32(vdw1); vdw2 = _f32(vdw2)
        d = SearchDesc()
        d.kind = kind
        d.cutoff = float(cutoff) if cutoff is not None else 0.0
        keep = []
        for name, arr in (("xyz1", xyz1), ("idx1", idx1), ("xyz2", xyz2), ("idx2", idx2), ("vdw1", vdw1),
                          ("vdw2", vdw2)):
            a, k = _addr(arr)
            setattr(d, name, a)
            keep.append(k)
        d.natoms1 = 0 if xyz1 is None else xyz1.shape[0] if xyz1.ndim == 2 else xyz1.shape[0] // 3
        d.natoms2 = 0 if xyz2 is None else xyz2.shape[0] if xyz2.ndim == 2 else xyz2.shape[0] // 3
        d.n1 = 0 if idx1 is None else idx1.shape[0]
        d.n2 = 0 if idx2 is None else idx2.shape[0]
        d.ids_local = 1 if ids_local else 0
        if box is not None:
            b9 = box.colmajor9() if isinstance(box, PeriodicBox) else np.ascontiguousarray(
                np.asarray(box, np.float32).reshape(3, 3).T).reshape(9)
            keep.append(b9)
            d.box9 = b9.ctypes.data
        d.pbc = pbc_mask(pbc)
        if lower is not None:
            lo = np.ascontiguousarray(lower, np.float32); up = np.ascontiguousarray(upper, np.float32)
            keep += [lo, up]
            d.lower3 = lo.ctypes.data
            d.upper3 = up.ctypes.data
        return d, keep

    def search_count(self, kind, cutoff, xyz1, idx1=None, xyz2=None, idx2=None, box=None, pbc=0, vdw1=None,
                     vdw2=None, ids_local=False, lower=None, upper=None) -> int:
        d, keep = self._search_desc(kind, cutoff, xyz1, idx1, xyz2, idx2, box, pbc, vdw1, vdw2, ids_local, lower, upper)
        cnt = C.c_uint64(0)
        check(self.lib.molar_hip_search_count(self.ctx, C.byref(d), C.byref(cnt)))
        self._keep = keep
        return int(cnt.value)

    def make_search_desc(self, kind, cutoff, xyz1, **kw):
        """A reusable search description for per-frame loops: build once, point `desc.xyz1` (and xyz2) at each new
        frame (`desc.xyz1 = frame.data_ptr()`), run with search_resident_desc / search_count_desc.  Returns
        (desc, keepalive)."""
        return self._search_desc(kind, cutoff, xyz1, **kw)

    def search_resident_desc(self, desc):
        cnt = C.c_uint64(0); p = C.c_void_p(); dd = C.c_void_p()
        check(self.lib.molar_hip_search_resident(self.ctx, C.byref(desc), C.byref(cnt), C.byref(p), C.byref(dd)))
        return int(cnt.value), p.value, dd.value

    def search_cell_kernels(self):
        """molar_hip_search_cell_kernels: (lanes, occupied cells of the two grids) of the context's last fixed-cutoff search -
        lanes 16 / 32 = small-cell kernels, 0 = regular ones."""
        lanes = C.c_int32(-1)
        occ = (C.c_uint64 * 2)()
        check(self.lib.molar_hip_search_cell_kernels(self.ctx, C.byref(lanes), occ))
        return int(lanes.value), (int(occ[0]), int(occ[1]))

    def search_slot_counts(self):
        """molar_hip_search_slot_counts: (slots the plan of the context's last search produced, slots that 64 consecutive rows per
        plan entry would have given).  The first is smaller where slots are cut from live rows; equal everywhere else."""
        slots, rows = C.c_uint64(0), C.c_uint64(0)
        check(self.lib.molar_hip_search_slot_counts(self.ctx, C.byref(slots), C.byref(rows)))
        return int(slots.value), int(rows.value)

    def search_resident_planes(self, want_dist=True):
        """molar_hip_search_resident_planes: want_dist=False makes the resident searches fill the (i, j) plane only
        (DistanceSearchOutput of (usize, usize)); the distance addresses they return are then None."""
        check(self.lib.molar_hip_search_resident_planes(self.ctx, 1 if want_dist else 0))

    def search_resident_begin(self, desc):
        """Enqueue a whole resident search and return its ticket without waiting (molar_hip_search_resident_begin).
        `desc` (and what it points to) must stay alive and unchanged until search_resident_end(ticket)."""
        t = C.c_int32(-1)
        check(self.lib.molar_hip_search_resident_begin(self.ctx, C.byref(desc), C.byref(t)))
        return int(t.value)

    def search_resident_end(self, ticket):
        """Wait for the search behind `ticket`; returns (count, pairs_device_address, dist_device_address)."""
        cnt = C.c_uint64(0); p = C.c_void_p(); dd = C.c_void_p()
        check(self.lib.molar_hip_search_resident_end(self.ctx, C.c_int32(ticket), C.byref(cnt), C.byref(p), C.byref(dd)))
        return int(cnt.value), p.value, dd.value

    def search_resident(self, kind, cutoff, xyz1, idx1=None, xyz2=None, idx2=None, box=None, pbc=0, vdw1=None,
                        vdw2=None, ids_local=False, lower=None, upper=None):
        """Count + fill into engine-owned device buffers with a single host round trip
        (molar_hip_search_resident).  Returns (count, pairs_device_address, dist_device_address)."""
        d, keep = self._search_desc(kind, cutoff, xyz1, idx1, xyz2, idx2, box, pbc, vdw1, vdw2, ids_local, lower, upper)
        cnt = C.c_uint64(0); p = C.c_void_p(); dd = C.c_void_p()
        check(self.lib.molar_hip_search_resident(self.ctx, C.byref(d), C.byref(cnt), C.byref(p), C.byref(dd)))
        self._keep = keep
        return int(cnt.value), p.value, dd.value

    def search_fill(self, count):
        pairs = np.empty((count, 2), np.uint32)
        dist = np.empty(count, np.float32)
        check(self.lib.molar_hip_search_fill(self.ctx, pairs.ctypes.data, dist.ctypes.data))
        return pairs, dist

    def search_fill_usize(self, count):
        i = np.empty(count, np.uint64); j = np.empty(count, np.uint64); d = np.empty(count, np.float32)
        check(self.lib.molar_hip_search_fill_usize(self.ctx, i.ctypes.data, j.ctypes.data, d.ctypes.data))
        return i, j, d

    def within_set(self, cutoff, xyz1, idx1=None, xyz2=None, idx2=None, box=None, pbc=0, ids_local=False, lower=None,
                   upper=None, device_out=None):
        """`within` as the set its callers keep (molar_hip_within_count + _fill): sorted, de-duplicated ids of the atoms of
        set 1 with an atom of set 2 within the cutoff - np.unique of the stream search_count(SEARCH_WITHIN) +
        search_fill_ids returns, without the stream.  Returns a uint64 array (or, with `device_out` = a callable that
        allocates a device int64 tensor of a given length, that tensor)."""
        d, keep = self._search_desc(SEARCH_WITHIN, cutoff, xyz1, idx1, xyz2, idx2, box, pbc, None, None, ids_local, lower, upper)
        cnt = C.c_uint64(0)
        check(self.lib.molar_hip_within_count(self.ctx, C.byref(d), C.byref(cnt)))
        self._keep = keep
        n = int(cnt.value)
        if device_out is not None:
            out = device_out(n)
            if n:
                check(self.lib.molar_hip_within_fill(self.ctx, out.data_ptr()))
            return out
        ids = np.empty(n, np.uint64)
        if n:
            check(self.lib.molar_hip_within_fill(self.ctx, ids.ctypes.data))
        return ids

    def search_connectivity(self, cutoff, xyz, idx=None, box=None, pbc=0, ids_local=True):
        """SearchConnectivity::from_iter over the single-selection search (connectivity.rs:19-35), built on the device from
        the resident pair list (molar_hip_search_connectivity / _fill): CSR (offsets uint64[rows + 1], neigh uint64[2 * pairs])
        with every list in the reference's push order; rows = len(selection) for local ids, natoms for global ones."""
        d, keep = self._search_desc(SEARCH_SINGLE, cutoff, xyz, idx, None, None, box, pbc, None, None, ids_local, None, None)
        rows, ent = C.c_uint64(0), C.c_uint64(0)
        check(self.lib.molar_hip_search_connectivity(self.ctx, C.byref(d), C.byref(rows), C.byref(ent)))
        self._keep = keep
        off = np.empty(rows.value + 1, np.uint64)
        nb = np.empty(max(ent.value, 1), np.uint64)
        check(self.lib.molar_hip_search_connectivity_fill(self.ctx, off.ctypes.data, nb.ctypes.data))
        return off, nb[:ent.value]

    def within_hold(self, on=True):
        """molar_hip_within_hold: while on, within_set calls that name the same first set (same array / tensor, same index,
        same box) and come to the same grid reuse its staged coordinates and its grid.  The caller promises not to change
        those coordinates meanwhile."""
        check(self.lib.molar_hip_within_hold(self.ctx, 1 if on else 0))

    def search_fill_ids(self, count):
        ids = np.empty(count, np.uint64)
        check(self.lib.molar_hip_search_fill_ids(self.ctx, ids.ctypes.data))
        return ids

    def search_fill_device(self):
        """Fill ctx-owned device buffers; returns (pairs_ptr, dist_ptr) device addresses."""
        p = C.c_void_p(); d = C.c_void_p()
        check(self.lib.molar_hip_search_fill_device(self.ctx, C.byref(p), C.byref(d)))
        return p.value, d.value

    def search_fill_into(self, pairs_t, dist_t):
        """Fill caller-owned torch CUDA tensors (uint32/int32 [N,2], float32 [N]) in place."""
        pa, _ = _addr(pairs_t); da, _ = _addr(dist_t)
        check(self.lib.molar_hip_search_fill(self.ctx, pa, da))

    # ------------------------------------------------------------ search, f64 build of MolAR (Float = f64)
    def search_f64(self, kind, cutoff, xyz1, idx1=None, xyz2=None, idx2=None, box=None, pbc=0, vdw1=None, vdw2=None,
                   ids_local=False, lower=None, upper=None, device_out=False, out=None):
        """The distance_search drivers with every operation in double (molar_hip_search_count_f64 + fill): returns
        (i, j, d) as uint64 / uint64 / float64 arrays in the reference's order, or the uint64 ids for SEARCH_WITHIN.
        Coordinates, indices and radii may be torch tensors in HBM (used in place); device_out=True leaves the result
        there too (int64 / int64 / float64 tensors); `out` = (i, j, d) device tensors of at least the result's length to fill
        instead of fresh ones (views of the result's length are returned)."""
        d, keep = _search_desc_f64(kind, cutoff, xyz1, idx1, xyz2, idx2, box, pbc, vdw1, vdw2, ids_local, lower, upper)
        n = C.c_uint64()
        check(self.lib.molar_hip_search_count_f64(self.ctx, C.byref(d), C.byref(n)))
        n = int(n.value)
        if device_out:
            import torch
            dev = torch.device("cuda", self.device)
            if kind == SEARCH_WITHIN:
                ids = torch.empty(n, dtype=torch.int64, device=dev)
                if n:
                    check(self.lib.molar_hip_search_fill_ids_f64(self.ctx, ids.data_ptr()))
                return ids
            if out is not None:
                if min(len(out[0]), len(out[1]), len(out[2])) < n:
                    raise ValueError("search_f64: `out` tensors are shorter than the result")
                i, j, dist = out[0][:n], out[1][:n], out[2][:n]
            else:
                i = torch.empty(n, dtype=torch.int64, device=dev); j = torch.empty(n, dtype=torch.int64, device=dev)
                dist = torch.empty(n, dtype=torch.float64, device=dev)
            if n:
                check(self.lib.molar_hip_search_fill_f64(self.ctx, i.data_ptr(), j.data_ptr(), dist.data_ptr()))
            return i, j, dist
        if kind == SEARCH_WITHIN:
            ids = np.empty(n, np.uint64)
            check(self.lib.molar_hip_search_fill_ids_f64(self.ctx, ids.ctypes.data))
            return ids
        i = np.empty(n, np.uint64); j = np.empty(n, np.uint64); dist = np.empty(n, np.float64)
        check(self.lib.molar_hip_search_fill_f64(self.ctx, i.ctypes.data, j.ctypes.data, dist.ctypes.data))
        return i, j, dist

    def within_set_f64(self, cutoff, xyz1, idx1=None, xyz2=None, idx2=None, box=None, pbc=0, ids_local=False, lower=None,
                       upper=None, device_out=None):
        """`within` as the set its callers keep, every operation in double (molar_hip_within_count_f64 + _fill_f64): sorted,
        de-duplicated ids of the atoms of set 1 with an atom of set 2 within the cutoff - np.unique of what
        search_f64(SEARCH_WITHIN) returns, without the stream.  Returns a uint64 array (or, with `device_out` = a callable
        that allocates a device int64 tensor of a given length, that tensor).  Invalidates the cached f64 search."""
        d, keep = _search_desc_f64(SEARCH_WITHIN, cutoff, xyz1, idx1, xyz2, idx2, box, pbc, None, None, ids_local, lower, upper)
        cnt = C.c_uint64(0)
        check(self.lib.molar_hip_within_count_f64(self.ctx, C.byref(d), C.byref(cnt)))
        n = int(cnt.value)
        if device_out is not None:
            out = device_out(n)
            if n:
                check(self.lib.molar_hip_within_fill_f64(self.ctx, out.data_ptr()))
            return out
        ids = np.empty(n, np.uint64)
        check(self.lib.molar_hip_within_fill_f64(self.ctx, ids.ctypes.data))
        return ids

    def search_connectivity_f64(self, cutoff, xyz, idx=None, box=None, pbc=0, ids_local=True):
        """SearchConnectivity::from_iter over the f64 single-selection search (molar_hip_search_connectivity_f64, filled by
        molar_hip_search_connectivity_fill): CSR (offsets uint64[rows + 1], neigh uint64[2 * pairs]) with every list in the
        reference's push order; rows = len(selection) for local ids, natoms for global ones."""
        d, keep = _search_desc_f64(SEARCH_SINGLE, cutoff, xyz, idx, None, None, box, pbc, None, None, ids_local, None, None)
        rows, ent = C.c_uint64(0), C.c_uint64(0)
        check(self.lib.molar_hip_search_connectivity_f64(self.ctx, C.byref(d), C.byref(rows), C.byref(ent)))
        off = np.empty(rows.value + 1, np.uint64)
        nb = np.empty(max(ent.value, 1), np.uint64)
        check(self.lib.molar_hip_search_connectivity_fill(self.ctx, off.ctypes.data, nb.ctypes.data))
        return off, nb[:ent.value]

    def search_histogram_f64(self, kind, cutoff, hmin, hmax, nbins, xyz1, idx1=None, xyz2=None, idx2=None, box=None, pbc=0,
                             vdw1=None, vdw2=None, bins=None, want_count=True):
        """molar_hip_search_histogram_f64: the fused histogram with every operation in double - the pairs and distances of
        search_f64 for the same request, each through the f64 Histogram1D::add_one, no pair list.  Inputs as for search_f64
        (float64 numpy or CUDA tensors, used in place; `box` a 3x3 matrix with the box vectors as columns).  `bins`
        (uint64[nbins] numpy or an int64 CUDA tensor) is accumulated into.  Returns (bins, number_of_pairs); with device bins
        and want_count=False the call may return before the GPU is done (count None): synchronize() before reading.  The
        call invalidates the cached f64 search."""
        d, keep = _search_desc_f64(kind, cutoff, xyz1, idx1, xyz2, idx2, box, pbc, vdw1, vdw2)
        if bins is None:
            bins = np.zeros(nbins, np.uint64)
        ba, kb = _addr(bins)
        cnt = C.c_uint64(0)
        check(self.lib.molar_hip_search_histogram_f64(self.ctx, C.byref(d), float(hmin), float(hmax), int(nbins), ba,
                                                      C.byref(cnt) if want_count else None))
        self._keep = keep + [kb]
        return bins, (int(cnt.value) if want_count else None)

    def search_histogram_frames_f64(self, kind, cutoff, hmin, hmax, nbins, frames, idx1=None, box=None, pbc=0, bins=None,
                                    frames2=None, idx2=None):
        """molar_hip_search_histogram_frames_f64: `frames` = [nframes, natoms, 3] float64 (numpy, or a CUDA tensor - a window
        of a larger buffer with a gap between frames is passed without a copy) through the f64 fused histogram; the same sums
        as nframes calls of search_histogram_f64.  `box`: one 3x3 matrix for all frames or [nframes, 3, 3] (box vectors as
        columns).  SEARCH_DOUBLE / _VDW: the second set is `idx2` of `frames2` (None: of the same frames).  With device bins
        the call may return before the GPU is done: synchronize() before reading."""
        def block(fr):
            if _is_torch(fr) and fr.ndim == 3 and fr.stride(2) == 1 and fr.stride(1) == 3:
                import torch
                if fr.dtype != torch.float64:
                    raise TypeError("search_histogram_frames_f64: frames must be float64")
                return fr, fr.data_ptr(), fr, int(fr.stride(0))
            if _is_torch(fr):
                fr = _f64(fr)
                return fr, fr.data_ptr(), fr, int(fr.shape[1]) * 3
            fr = np.ascontiguousarray(fr, np.float64)
            return fr, fr.ctypes.data, fr, int(fr.shape[1]) * 3
        frames, fa, k1, stride = block(frames)
        if frames.ndim != 3 or frames.shape[2] != 3:
            raise ValueError("search_histogram_frames_f64: frames must be [nframes, natoms, 3]")
        nframes = int(frames.shape[0])
        two = kind in (SEARCH_DOUBLE, SEARCH_DOUBLE_VDW)
        f2, stride2 = None, 0
        if two:
            f2, fa2, k2, stride2 = block(frames if frames2 is None else frames2)
            if int(f2.shape[0]) != nframes:
                raise ValueError("search_histogram_frames_f64: frames2 must have as many frames as frames")
        boxes_ptr, box0 = None, None
        keep = [k1]
        if box is not None:
            b = np.asarray(box.get_matrix() if isinstance(box, PeriodicBox) else box, np.float64)
            if b.ndim == 3:
                b9 = np.ascontiguousarray(np.transpose(b, (0, 2, 1))).reshape(nframes, 9)      # column-major per frame
                boxes_ptr = b9.ctypes.data
                keep.append(b9)
                box0 = b[0]
            else:
                box0 = b.reshape(3, 3)
        # the request of frame 0 (shapes, selections, box) - the library moves the coordinates on by the strides
        d, k0 = _search_desc_f64(kind, cutoff, frames[0], idx1, f2[0] if two else None, idx2 if two else None, box0, pbc)
        d.xyz1 = fa
        if two:
            d.xyz2 = fa2
            keep.append(k2)
        if bins is None:
            bins = np.zeros(nbins, np.uint64)
        ba, kb = _addr(bins)
        check(self.lib.molar_hip_search_histogram_frames_f64(self.ctx, C.byref(d), nframes, stride, stride2, boxes_ptr,
                                                             float(hmin), float(hmax), int(nbins), ba))
        self._keep = keep + k0 + [kb]
        return bins

    def grid_dims_f64(self):
        dims = (C.c_uint64 * 3)()
        check(self.lib.molar_hip_search_grid_dims_f64(self.ctx, dims))
        return tuple(int(x) for x in dims)

    def grid_dims(self):
        dims = (C.c_uint64 * 3)()
        check(self.lib.molar_hip_search_grid_dims(self.ctx, dims))
        return tuple(int(x) for x in dims)

    def search_histogram(self, kind, cutoff, hmin, hmax, nbins, xyz1, idx1=None, xyz2=None, idx2=None, box=None,
                         pbc=0, vdw1=None, vdw2=None, bins=None, want_count=True):
        """Consumer-fused search: every emitted distance goes through Histogram1D::add_one
        (molar_membrane/src/stats.rs:29-35); pairs are never materialised.  `bins` (uint64[nbins], numpy or a torch
        int64 CUDA tensor) is accumulated into, so frames can be summed.  Returns (bins, number_of_pairs).  With
        device-resident bins and want_count=False the call does not wait for the GPU (count is returned as None):
        the frames of a trajectory queue up back to back; synchronize() before reading the bins."""
        xyz1 = _f32(xyz1); xyz2 = _f32(xyz2); idx1 = _u64(idx1); idx2 = _u64(idx2)
        vdw1 = _f32(vdw1); vdw2 = _f32(vdw2)
        d = SearchDesc()
        d.kind = kind
        d.cutoff = float(cutoff) if cutoff is not None else 0.0
        keep = []
        for name, arr in (("xyz1", xyz1), ("idx1", idx1), ("xyz2", xyz2), ("idx2", idx2), ("vdw1", vdw1),
                          ("vdw2", vdw2)):
            a, k = _addr(arr)
            setattr(d, name, a)
            keep.append(k)
        d.natoms1 = 0 if xyz1 is None else xyz1.shape[0]
        d.natoms2 = 0 if xyz2 is None else xyz2.shape[0]
        d.n1 = 0 if idx1 is None else idx1.shape[0]
        d.n2 = 0 if idx2 is None else idx2.shape[0]
        if box is not None:
            ba, kb = self._box9(box)
            keep.append(kb)
            d.box9 = ba
        d.pbc = pbc_mask(pbc)
        if bins is None:
            bins = np.zeros(nbins, np.uint64)
        cnt = C.c_uint64(0)
        ba_, kb_ = _addr(bins)
        check(self.lib.molar_hip_search_histogram(self.ctx, C.byref(d), float(hmin), float(hmax), nbins,
                                                  ba_, C.byref(cnt) if want_count else None))
        self._keep = keep
        return bins, (int(cnt.value) if want_count else None)

    def search_histogram_frames(self, kind, cutoff, hmin, hmax, nbins, frames, idx1=None, box=None, pbc=0, bins=None, frames2=None, idx2=None):
        """molar_hip_search_histogram_frames: the frames of a trajectory block, `frames` = [nframes, natoms, 3] float32 (one
        contiguous array or CUDA tensor), through the fused histogram; the same sums as nframes calls of search_histogram.
        `box`: one 3x3 matrix for all frames or [nframes, 3, 3].  SEARCH_DOUBLE: the second set is `idx2` of `frames2` (None:
        of the same frames - two selections of one trajectory).  With frames, indices and bins in device memory the frames go
        through the GPU in groups that share their launches, and the call does not wait (synchronize() before reading)."""
        def block(fr):
            stride = None
            if _is_torch(fr) and fr.ndim == 3 and fr.stride(2) == 1 and fr.stride(1) == 3:
                import torch
                assert fr.dtype == torch.float32
                stride = int(fr.stride(0))          # frames with a gap between them (a window of a larger buffer): no copy
                fa, k = fr.data_ptr(), fr
            else:
                fr = _f32(fr)
                fa, k = _addr(fr)
            assert fr.ndim == 3 and fr.shape[2] == 3
            return fr, fa, k, (int(fr.shape[1]) * 3 if stride is None else stride)
        frames, fa, k1, stride = block(frames)
        idx1 = _u64(idx1)
        nframes, natoms = int(frames.shape[0]), int(frames.shape[1])
        d = SearchDesc()
        d.kind = kind
        d.cutoff = float(cutoff)
        ia, k2 = _addr(idx1)
        d.xyz1 = fa
        d.idx1 = ia
        d.natoms1 = natoms
        d.n1 = 0 if idx1 is None else idx1.shape[0]
        keep = [k1, k2]
        stride2 = 0
        if kind in (SEARCH_DOUBLE, SEARCH_DOUBLE_VDW):
            f2, fa2, k3, stride2 = block(frames if frames2 is None else frames2)
            assert int(f2.shape[0]) == nframes
            idx2 = _u64(idx2)
            ia2, k4 = _addr(idx2)
            d.xyz2 = fa2
            d.idx2 = ia2
            d.natoms2 = int(f2.shape[1])
            d.n2 = 0 if idx2 is None else idx2.shape[0]
            keep += [k3, k4]
        boxes_ptr = None
        if box is not None:
            b = np.asarray(box.get_matrix() if isinstance(box, PeriodicBox) else box, np.float32)
            if b.ndim == 3:
                b9 = np.ascontiguousarray(np.transpose(b, (0, 2, 1))).reshape(nframes, 9)      # column-major per frame
                boxes_ptr = b9.ctypes.data
                d.box9 = boxes_ptr
            else:
                b9 = np.ascontiguousarray(b.reshape(3, 3).T).reshape(9)
                d.box9 = b9.ctypes.data
            keep.append(b9)
        d.pbc = pbc_mask(pbc)
        if bins is None:
            bins = np.zeros(nbins, np.uint64)
        ba_, kb_ = _addr(bins)
        check(self.lib.molar_hip_search_histogram_frames(self.ctx, C.byref(d), nframes, stride, stride2, boxes_ptr, float(hmin), float(hmax),
                                                         nbins, ba_))
        self._keep = keep
        return bins

    # ------------------------------------------------------------ contact counts
    def _contacts_desc(self, kind, cutoff, xyz1, idx1, xyz2, idx2, pbc):
        d = SearchDesc()
        d.kind = kind
        d.cutoff = float(cutoff)
        keep = []
        for name, arr in (("xyz1", xyz1), ("idx1", idx1), ("xyz2", xyz2), ("idx2", idx2)):
            a, k = _addr(arr)
            setattr(d, name, a)
            keep.append(k)
        d.natoms1 = 0 if xyz1 is None else xyz1.shape[-2]
        d.natoms2 = 0 if xyz2 is None else xyz2.shape[-2]
        d.n1 = 0 if idx1 is None else idx1.shape[0]
        d.n2 = 0 if idx2 is None else idx2.shape[0]
        d.pbc = pbc_mask(pbc)
        return d, keep

    @staticmethod
    def _contacts_out(arr, want, shape, like, dtype64=True):
        """An output of the contacts calls: the caller's array, or zeros (a CUDA tensor when the coordinates are one)."""
        if arr is not None or not want:
            return arr
        if _is_torch(like):
            import torch
            return torch.zeros(shape, dtype=torch.int64 if dtype64 else torch.int32, device=like.device)
        return np.zeros(shape, np.uint64 if dtype64 else np.uint32)

    def search_contacts(self, kind, cutoff, xyz1, idx1=None, xyz2=None, idx2=None, box=None, pbc=0, group1=None, ngroups1=0,
                        group2=None, ngroups2=0, deg1=None, deg2=None, cmap=None, want_deg=True, want_map=None, want_count=True):
        """molar_hip_search_contacts: per-atom contact counts and the group x group contact matrix of the pair list, fused
        into the pair loop (no pair is written).  `group1` / `group2`: one label per SELECTED atom.  deg1 / deg2 / cmap
        (uint64 numpy or int64 CUDA tensors) are accumulated into; missing ones are made as zeros when wanted (want_map
        defaults to "labels were given"), CUDA tensors when xyz1 is one.  SINGLE: deg1 counts both members, deg2 stays
        None and only the upper triangle of cmap is used.  The counts include the reference list's duplicates
        (include/molar_hip.h).  Returns a `Contacts`; with every output on the device and want_count=False the call does
        not wait (synchronize() before reading)."""
        xyz1 = _f32(xyz1); xyz2 = _f32(xyz2); idx1 = _u64(idx1); idx2 = _u64(idx2)
        group1 = _u32(group1); group2 = _u32(group2)
        two = kind == SEARCH_DOUBLE
        d, keep = self._contacts_desc(kind, cutoff, xyz1, idx1, xyz2, idx2, pbc)
        if box is not None:
            ba, kb = self._box9(box)
            keep.append(kb)
            d.box9 = ba
        n1 = d.n1 if idx1 is not None else d.natoms1
        n2 = d.n2 if idx2 is not None else d.natoms2
        if want_map is None:
            want_map = group1 is not None
        deg1 = self._contacts_out(deg1, want_deg, (n1,), xyz1)
        deg2 = self._contacts_out(deg2, want_deg and two, (n2,), xyz1)
        cmap = self._contacts_out(cmap, want_map, (int(ngroups1), int(ngroups2) if two else int(ngroups1)), xyz1)
        g = ContactGroups()
        (g.group1, k1), (g.group2, k2) = _addr(group1), _addr(group2)
        g.ngroups1, g.ngroups2 = int(ngroups1), int(ngroups2)
        keep += [k1, k2]
        cnt = C.c_uint64(0)
        check(self.lib.molar_hip_search_contacts(self.ctx, C.byref(d), C.byref(g) if group1 is not None else None, _addr(deg1)[0],
                                                 _addr(deg2)[0], _addr(cmap)[0], C.byref(cnt) if want_count else None))
        self._keep = keep
        return Contacts(int(cnt.value) if want_count else None, deg1, deg2, cmap)

    def search_contacts_frames(self, kind, cutoff, frames, idx1=None, box=None, pbc=0, frames2=None, idx2=None, group1=None, ngroups1=0,
                               group2=None, ngroups2=0, deg1=None, deg2=None, cmap=None, occupancy=None, want_deg=True, want_map=None,
                               want_occupancy=None):
        """molar_hip_search_contacts_frames: `frames` = [nframes, natoms, 3] float32 (numpy or a CUDA tensor, frames may have a
        gap between them) through search_contacts - the same sums as nframes calls - plus `occupancy` (uint32 / int32, the
        map's shape): the number of frames in which each group pair was in contact.  `box`: one 3x3 matrix or
        [nframes, 3, 3].  SEARCH_DOUBLE: the second set is `idx2` of `frames2` (None: of the same frames).  Returns a
        `Contacts` with count None; synchronize() before reading device outputs."""
        def block(fr):
            stride = None
            if _is_torch(fr) and fr.ndim == 3 and fr.stride(2) == 1 and fr.stride(1) == 3:
                import torch
                assert fr.dtype == torch.float32
                stride = int(fr.stride(0))
                fa, k = fr.data_ptr(), fr
            else:
                fr = _f32(fr)
                fa, k = _addr(fr)
            assert fr.ndim == 3 and fr.shape[2] == 3
            return fr, fa, k, (int(fr.shape[1]) * 3 if stride is None else stride)
        frames, fa, k1, stride = block(frames)
        idx1 = _u64(idx1); idx2 = _u64(idx2)
        group1 = _u32(group1); group2 = _u32(group2)
        nframes = int(frames.shape[0])
        two = kind == SEARCH_DOUBLE
        f2, fa2, k3, stride2 = (None, None, None, 0)
        if kind != SEARCH_SINGLE:
            f2, fa2, k3, stride2 = block(frames if frames2 is None else frames2)
            assert int(f2.shape[0]) == nframes
        d, keep = self._contacts_desc(kind, cutoff, None, idx1, None, idx2, pbc)
        d.xyz1, d.xyz2 = fa, fa2
        d.natoms1 = int(frames.shape[1])
        d.natoms2 = 0 if f2 is None else int(f2.shape[1])
        keep += [k1, k3]
        boxes_ptr = None
        if box is not None:
            b = np.asarray(box.get_matrix() if isinstance(box, PeriodicBox) else box, np.float32)
            if b.ndim == 3:
                b9 = np.ascontiguousarray(np.transpose(b, (0, 2, 1))).reshape(nframes, 9)      # column-major per frame
                boxes_ptr = b9.ctypes.data
                d.box9 = boxes_ptr
            else:
                b9 = np.ascontiguousarray(b.reshape(3, 3).T).reshape(9)
                d.box9 = b9.ctypes.data
            keep.append(b9)
        n1 = d.n1 if idx1 is not None else d.natoms1
        n2 = d.n2 if idx2 is not None else d.natoms2
        if want_map is None:
            want_map = group1 is not None
        if want_occupancy is None:
            want_occupancy = group1 is not None
        shape = (int(ngroups1), int(ngroups2) if two else int(ngroups1))
        deg1 = self._contacts_out(deg1, want_deg, (n1,), frames)
        deg2 = self._contacts_out(deg2, want_deg and two, (n2,), frames)
        cmap = self._contacts_out(cmap, want_map, shape, frames)
        occupancy = self._contacts_out(occupancy, want_occupancy, shape, frames, dtype64=False)
        g = ContactGroups()
        (g.group1, g1k), (g.group2, g2k) = _addr(group1), _addr(group2)
        g.ngroups1, g.ngroups2 = int(ngroups1), int(ngroups2)
        keep += [g1k, g2k]
        check(self.lib.molar_hip_search_contacts_frames(self.ctx, C.byref(d), C.byref(g) if group1 is not None else None, nframes, stride,
                                                        stride2, boxes_ptr, _addr(deg1)[0], _addr(deg2)[0], _addr(cmap)[0],
                                                        _addr(occupancy)[0]))
        self._keep = keep
        return Contacts(None, deg1, deg2, cmap, occupancy)

    # ------------------------------------------------------------ connected components
    @staticmethod
    def _clusters_out(want, shape, like, dtype64=False):
        """An output of the clusters calls (overwritten by the engine): a CUDA tensor when the coordinates are one."""
        if not want:
            return None
        if _is_torch(like):
            import torch
            return torch.zeros(shape, dtype=torch.int64 if dtype64 else torch.int32, device=like.device)
        return np.zeros(shape, np.uint64 if dtype64 else np.uint32)

    def search_clusters(self, cutoff, xyz, idx=None, box=None, pbc=0, group=None, ngroups=0, want_members=True):
        """molar_hip_search_clusters: the connected components of the contact graph of one selection, fused into the pair loop
        (no pair is written).  The particles are the selected atoms (ids = positions in the selection) or, with `group` (one
        label per SELECTED atom) and `ngroups`, the groups; two particles are joined when distance_search_single(_pbc) lists a
        pair with its ends in them.  Components are numbered in the order of their smallest particle.  Returns a `Clusters`
        (numpy uint32 / uint64 arrays, int32 / int64 CUDA tensors when `xyz` is one); the call is complete when it returns."""
        xyz = _f32(xyz); idx = _u64(idx); group = _u32(group)
        d, keep = self._contacts_desc(SEARCH_SINGLE, cutoff, xyz, idx, None, None, pbc)
        if box is not None:
            ba, kb = self._box9(box)
            keep.append(kb)
            d.box9 = ba
        n = d.n1 if idx is not None else d.natoms1
        npart = int(ngroups) if group is not None else int(n)
        comp_of = self._clusters_out(True, (npart,), xyz)
        sizes = self._clusters_out(True, (npart,), xyz)
        offsets = self._clusters_out(want_members, (npart + 1,), xyz, dtype64=True)
        members = self._clusters_out(want_members, (npart,), xyz)
        g = ContactGroups()
        g.group1, k1 = _addr(group)
        g.ngroups1 = int(ngroups)
        keep.append(k1)
        cnt = C.c_uint32(0)
        check(self.lib.molar_hip_search_clusters(self.ctx, C.byref(d), C.byref(g) if group is not None else None, _addr(comp_of)[0],
                                                 _addr(sizes)[0], _addr(offsets)[0], _addr(members)[0], C.byref(cnt)))
        self._keep = keep
        c = int(cnt.value)
        return Clusters(c, comp_of, sizes[:c], None if offsets is None else offsets[:c + 1], members)

    def search_clusters_frames(self, cutoff, frames, idx=None, box=None, pbc=0, group=None, ngroups=0, size_hist=None, want_comp_of=False):
        """molar_hip_search_clusters_frames: `frames` = [nframes, natoms, 3] float32 (numpy or a CUDA tensor) through
        search_clusters, one frame after the other.  `box`: one 3x3 matrix or [nframes, 3, 3].  `size_hist` (uint64 numpy or
        int64 CUDA tensor of P + 1 entries) is ADDED INTO - size_hist[s] += components of s particles, summed over the frames -
        and made as zeros when None.  Returns a `ClustersBlock`: ncomponents[nframes], largest[nframes], size_hist and, with
        want_comp_of, comp_of[nframes, P] in each frame's canonical numbering."""
        stride = None
        if _is_torch(frames) and frames.ndim == 3 and frames.stride(2) == 1 and frames.stride(1) == 3:
            import torch
            assert frames.dtype == torch.float32
            stride = int(frames.stride(0))
            fa, k1 = frames.data_ptr(), frames
        else:
            frames = _f32(frames)
            fa, k1 = _addr(frames)
        assert frames.ndim == 3 and frames.shape[2] == 3
        if stride is None:
            stride = int(frames.shape[1]) * 3
        idx = _u64(idx); group = _u32(group)
        nframes = int(frames.shape[0])
        d, keep = self._contacts_desc(SEARCH_SINGLE, cutoff, None, idx, None, None, pbc)
        d.xyz1 = fa
        d.natoms1 = int(frames.shape[1])
        keep.append(k1)
        boxes_ptr = None
        if box is not None:
            b = np.asarray(box.get_matrix() if isinstance(box, PeriodicBox) else box, np.float32)
            if b.ndim == 3:
                b9 = np.ascontiguousarray(np.transpose(b, (0, 2, 1))).reshape(nframes, 9)      # column-major per frame
                boxes_ptr = b9.ctypes.data
                d.box9 = boxes_ptr
            else:
                b9 = np.ascontiguousarray(b.reshape(3, 3).T).reshape(9)
                d.box9 = b9.ctypes.data
            keep.append(b9)
        n = d.n1 if idx is not None else d.natoms1
        npart = int(ngroups) if group is not None else int(n)
        ncomp = self._clusters_out(True, (nframes,), frames)
        largest = self._clusters_out(True, (nframes,), frames)
        if size_hist is None:
            size_hist = self._clusters_out(True, (npart + 1,), frames, dtype64=True)
        comp_of = self._clusters_out(want_comp_of, (nframes, npart), frames)
        g = ContactGroups()
        g.group1, kg = _addr(group)
        g.ngroups1 = int(ngroups)
        keep.append(kg)
        check(self.lib.molar_hip_search_clusters_frames(self.ctx, C.byref(d), C.byref(g) if group is not None else None, nframes, stride,
                                                        boxes_ptr, _addr(ncomp)[0], _addr(largest)[0], _addr(size_hist)[0],
                                                        _addr(comp_of)[0]))
        self._keep = keep
        return ClustersBlock(ncomp, largest, size_hist, comp_of)

    def clusters_counters(self, enable):
        """molar_hip_search_clusters_counters: returns [hits, hits that reached the forest, CAS, atomicMin] of the clusters
        calls since the counters were switched on, then switches them on (zeroed) or off.  For measurements."""
        out = (C.c_uint64 * 4)()
        check(self.lib.molar_hip_search_clusters_counters(self.ctx, 1 if enable else 0, out))
        return [int(v) for v in out]

    # ------------------------------------------------------------ hydrogen bonds
    def _hbonds_request(self, donors, hydrogens, acceptors, cutoff, pbc, angle, angle_kind, natoms):
        donors = _sel(donors); acceptors = _sel(acceptors)
        d, keep = self._contacts_desc(SEARCH_DOUBLE, cutoff, None, donors, None, acceptors, pbc)
        d.natoms1 = d.natoms2 = int(natoms)
        n1 = d.n1 if donors is not None else d.natoms1
        n2 = d.n2 if acceptors is not None else d.natoms2
        off, hidx = hydrogens_csr(hydrogens, n1)
        kind = {"dha": HBOND_DHA_MIN, "hda": HBOND_HDA_MAX}.get(angle_kind, angle_kind)
        (oa, ko), (ha, kh) = _addr(off), _addr(hidx)
        keep += [ko, kh]
        req = (oa, ha if hidx.shape[0] else None, int(hidx.shape[0]), int(kind), float(angle))
        return d, keep, n1, n2, req

    @staticmethod
    def _hbonds_groups(group1, ngroups1, group2, ngroups2, keep):
        group1 = _u32(group1); group2 = _u32(group2)
        if group1 is None:
            return None
        g = ContactGroups()
        (g.group1, k1), (g.group2, k2) = _addr(group1), _addr(group2)
        g.ngroups1, g.ngroups2 = int(ngroups1), int(ngroups2)
        keep += [k1, k2, g]
        return C.byref(g)

    def hbonds(self, xyz, donors, hydrogens, acceptors, box=None, pbc=7, cutoff=0.35, angle=150.0, angle_kind="dha", max_ha=0.0,
               group1=None, ngroups1=0, group2=None, ngroups2=0, don_count=None, acc_count=None, cmap=None, want_counts=True,
               want_map=None, want_columns=True):
        """Hydrogen bonds of one frame (molar_hip_hbonds_counts + _fill; the definition is in include/molar_hip.h).  `donors` /
        `acceptors`: atom indices into `xyz` (None: every atom); `hydrogens`: one atom index per donor, a list of lists, or
        the CSR (offsets, idx) over the donors.  angle_kind "dha": angle(D-H-A) >= angle; "hda": angle(H-D-A) <= angle;
        max_ha > 0 adds |H-A| <= max_ha.  `pbc` counts only with a box.  don_count / acc_count / cmap (uint64 numpy or int64
        CUDA tensors) are accumulated into; missing ones are made as zeros when wanted (CUDA tensors when xyz is one).
        Returns an `HBonds`; with xyz a CUDA tensor its arrays are CUDA tensors (triples int32, columns float64)."""
        xyz = _f32(xyz)
        d, keep, n1, n2, req = self._hbonds_request(donors, hydrogens, acceptors, cutoff, pbc, angle, angle_kind, xyz.shape[-2])
        d.xyz1 = d.xyz2 = _addr(xyz)[0]
        keep.append(xyz)
        if box is not None:
            ba, kb = self._box9(box)
            keep.append(kb)
            d.box9 = ba
        if want_map is None:
            want_map = group1 is not None
        don_count = self._contacts_out(don_count, want_counts, (n1,), xyz)
        acc_count = self._contacts_out(acc_count, want_counts, (n2,), xyz)
        cmap = self._contacts_out(cmap, want_map, (int(ngroups1), int(ngroups2)), xyz)
        g = self._hbonds_groups(group1, ngroups1, group2, ngroups2, keep)
        cnt = C.c_uint64(0)
        check(self.lib.molar_hip_hbonds_counts(self.ctx, C.byref(d), req[0], req[1], req[2], req[3], req[4], float(max_ha), g,
                                               _addr(don_count)[0], _addr(acc_count)[0], _addr(cmap)[0], C.byref(cnt)))
        self._keep = keep
        n = int(cnt.value)
        triples, cols = _hbonds_arrays(n, xyz, 3 if want_columns else 0)
        check(self.lib.molar_hip_hbonds_fill(self.ctx, _addr(triples)[0] if n else None, *[_addr(a)[0] if n else None for a in cols]))
        cols += [None] * (3 - len(cols))
        return HBonds(n, triples, cols[0], cols[1], cols[2], don_count, acc_count, cmap)

    def hbonds_frames(self, frames, donors, hydrogens, acceptors, box=None, pbc=7, cutoff=0.35, angle=150.0, angle_kind="dha", max_ha=0.0,
                      group1=None, ngroups1=0, group2=None, ngroups2=0, don_count=None, acc_count=None, cmap=None, want_counts=True,
                      want_map=None):
        """Hydrogen bonds of a block of frames (molar_hip_hbonds_frames + _frames_fill): `frames` = [nframes, natoms, 3] float32
        (numpy or a CUDA tensor, frames may have a gap between them), `box` one 3x3 matrix or [nframes, 3, 3].  The counts are
        summed over the frames.  Returns an `HBondsBlock`: the frames' lists one after the other (`frame_offsets`), the table
        of the block's distinct bonds with `occupancy` (frames present) and `bond_of_entry` (table row of every entry)."""
        if _is_torch(frames) and frames.ndim == 3 and frames.stride(2) == 1 and frames.stride(1) == 3:
            import torch
            assert frames.dtype == torch.float32
            stride = int(frames.stride(0))
        else:
            frames = _f32(frames)
            assert frames.ndim == 3 and frames.shape[2] == 3
            stride = int(frames.shape[1]) * 3
        nframes = int(frames.shape[0])
        d, keep, n1, n2, req = self._hbonds_request(donors, hydrogens, acceptors, cutoff, pbc, angle, angle_kind, frames.shape[1])
        d.xyz1 = d.xyz2 = frames.data_ptr() if _is_torch(frames) else frames.ctypes.data
        keep.append(frames)
        boxes_ptr = None
        if box is not None:
            b = np.asarray(box.get_matrix() if isinstance(box, PeriodicBox) else box, np.float32)
            if b.ndim == 3:
                b9 = np.ascontiguousarray(np.transpose(b, (0, 2, 1))).reshape(nframes, 9)      # column-major per frame
                boxes_ptr = b9.ctypes.data
            else:
                b9 = np.ascontiguousarray(b.reshape(3, 3).T).reshape(9)
            d.box9 = b9.ctypes.data
            keep.append(b9)
        if want_map is None:
            want_map = group1 is not None
        don_count = self._contacts_out(don_count, want_counts, (n1,), frames)
        acc_count = self._contacts_out(acc_count, want_counts, (n2,), frames)
        cmap = self._contacts_out(cmap, want_map, (int(ngroups1), int(ngroups2)), frames)
        g = self._hbonds_groups(group1, ngroups1, group2, ngroups2, keep)
        per_frame = np.zeros(nframes, np.uint64)
        total, unique = C.c_uint64(0), C.c_uint64(0)
        check(self.lib.molar_hip_hbonds_frames(self.ctx, C.byref(d), req[0], req[1], req[2], req[3], req[4], float(max_ha), nframes, stride,
                                               boxes_ptr, g, per_frame.ctypes.data if nframes else None, _addr(don_count)[0],
                                               _addr(acc_count)[0], _addr(cmap)[0], C.byref(total), C.byref(unique)))
        self._keep = keep
        n, rows = int(total.value), int(unique.value)
        frame_offsets = np.zeros(nframes + 1, np.uint64)
        triples, cols = _hbonds_arrays(n, frames, 3)
        table, _ = _hbonds_arrays(rows, frames, 0)
        boe, occ = _hbonds_u32(n, frames), _hbonds_u32(rows, frames)
        a = lambda x, m: _addr(x)[0] if m else None
        check(self.lib.molar_hip_hbonds_frames_fill(self.ctx, frame_offsets.ctypes.data, a(triples, n), a(cols[0], n), a(cols[1], n), a(cols[2], n),
                                                    a(boe, n), a(table, rows), a(occ, rows)))
        blk = HBondsBlock(per_frame, frame_offsets, triples, cols[0], cols[1], cols[2], table, occ, boe, don_count, acc_count, cmap)
        blk._engine = self
        blk._serial = self._hbonds_block_shape()[3]
        return blk

    # ------------------------------------------------------------ lifetime correlations
    def lifetimes(self, frame_offsets, row_of_entry, nrows, groups=None, ngroups=None, max_lag=None, origin_stride=1, gap=0,
                  want=LIFETIME_OUTPUTS):
        """Lifetime correlations of a sparse presence matrix frames x rows (molar_hip_lifetimes; the definition: molar_hip.h).
        `frame_offsets` [F + 1] (uint64 numpy or int64 CUDA tensor) and `row_of_entry` [E] (uint32 numpy or int32 CUDA tensor):
        the rows present in frame t are row_of_entry[frame_offsets[t] : frame_offsets[t + 1]].  `groups`: one label per row
        (None: one group; `ngroups` None: the largest label + 1 of a numpy array).  Lags 0 .. max_lag (None: F - 1), origins
        0, origin_stride, ...; `gap`: zero runs of at most this many frames between two present frames are filled first
        (MDAnalysis' intermittency).  `want`: the outputs to compute, of "inter", "cont", "run_hist", "events", "longest",
        "present".  Returns a `Lifetimes`; its arrays are CUDA tensors when row_of_entry is one (int64 / int32), numpy (uint64 /
        uint32) otherwise.  The call waits for its result."""
        off = _u64(frame_offsets)
        rows = _u32(row_of_entry)
        F = int(off.shape[0]) - 1
        (oa, k1), (ra, k2) = _addr(off), _addr(rows)
        if rows.shape[0] == 0:
            ra = None
        if _is_torch(off) or _is_torch(rows):
            import torch
            torch.cuda.current_stream().synchronize()      # torch made any contiguous copy on ITS stream
        call = lambda g, G, L, a: self.lib.molar_hip_lifetimes(self.ctx, oa, ra, F, int(nrows), g, G, L, int(origin_stride), int(gap), *a)
        return _lifetimes_call(call, F, int(nrows), groups, ngroups, max_lag, origin_stride, want, rows)

    def _hbonds_block_shape(self):
        """(nframes, rows, entries, serial) of the block the context holds (molar_hip_hbonds_frames_shape; NO_SEARCH without one)."""
        F, R, E, serial = C.c_size_t(0), C.c_size_t(0), C.c_size_t(0), C.c_uint64(0)
        check(self.lib.molar_hip_hbonds_frames_shape(self.ctx, C.byref(F), C.byref(R), C.byref(E), C.byref(serial)))
        return int(F.value), int(R.value), int(E.value), int(serial.value)

    def _hbonds_block_lifetimes(self, serial, like, groups, ngroups, max_lag, origin_stride, gap, want):
        # the outputs are sized by what the CONTEXT holds, and only when that is still the caller's block
        F, R, _, held = self._hbonds_block_shape()
        if held != serial:
            raise MolarHipError(ERR_NO_SEARCH, "HBondsBlock.lifetimes: the engine has computed another block since; its presence matrix "
                                                    "is gone (Engine.lifetimes on this block's frame_offsets / bond_of_entry still works)")
        call = lambda g, G, L, a: self.lib.molar_hip_hbonds_frames_lifetimes(self.ctx, g, G, L, int(origin_stride), int(gap), *a)
        return _lifetimes_call(call, F, R, groups, ngroups, max_lag, origin_stride, want, like)

    # ------------------------------------------------------------ surface area
    def sasa(self, xyz, vdw, idx=None, probe=0.14, npoints=960, want_exposed=False):
        """Per-atom solvent-accessible surface area by Shrake-Rupley (molar_hip_sasa; the definition is in
        include/molar_hip.h).  `vdw`: one radius per SELECTED atom, selection order.  Returns a `Sasa` (pymolar's
        sel.sasa(): .areas, .total_area; .exposed with want_exposed).  torch CUDA inputs are read in place and give
        torch CUDA results."""
        return _sasa_call(self.lib.molar_hip_sasa, self.ctx, _f32(xyz), _f32(vdw), _sel(idx), C.c_float(probe), npoints, want_exposed,
                          np.float32)

    def sasa_frames(self, frames, vdw, idx=None, probe=0.14, npoints=960):
        """molar_hip_sasa_frames over frames[F, natoms, 3] (numpy or torch CUDA): every frame is enqueued behind the one
        before it, one wait.  Returns (areas[F, n], totals[F]); frame by frame they equal `sasa` bit for bit."""
        return self._sasa_frames(frames, vdw, idx, probe, npoints, False)

    def sasa_vol(self, xyz, vdw, idx=None, probe=0.14, npoints=960, want_exposed=False):
        """`sasa` with the per-atom volumes (molar_hip_sasa_vol; Measure::sasa_vol, pymolar sel.sasa_vol()): the returned
        `Sasa` also has .volumes (each atom's ball inside its power cell, nm^3) and .total_volume (the union of the balls).
        Areas and exposed counts are those of `sasa` bit for bit."""
        return _sasa_call(self.lib.molar_hip_sasa_vol, self.ctx, _f32(xyz), _f32(vdw), _sel(idx), C.c_float(probe), npoints, want_exposed,
                          np.float32, want_volumes=True)

    def sasa_vol_frames(self, frames, vdw, idx=None, probe=0.14, npoints=960):
        """molar_hip_sasa_vol_frames over frames[F, natoms, 3] (numpy or torch CUDA), queued like `sasa_frames`.  Returns
        (areas[F, n], totals[F], volumes[F, n], total_volumes[F]); frame by frame they equal `sasa_vol` bit for bit."""
        return self._sasa_frames(frames, vdw, idx, probe, npoints, True)

    def _sasa_frames(self, frames, vdw, idx, probe, npoints, want_volumes):
        frames = _f32(frames)
        assert frames.ndim == 3 and frames.shape[2] == 3
        F, natoms = frames.shape[0], frames.shape[1]
        vdw = _f32(vdw); idx = _sel(idx)
        n = natoms if idx is None else idx.shape[0]
        assert vdw.shape[0] == n, "one radius per selected atom"

        def per_atom():
            if _is_torch(frames):
                import torch
                return torch.zeros((F, n), dtype=torch.float32, device=frames.device)
            return np.zeros((F, n), np.float32)
        areas, totals = per_atom(), np.zeros(F, np.float64)
        fa, k1 = _addr(frames); ia, k2 = _addr(idx); va, k3 = _addr(vdw); aa, k4 = _addr(areas)
        if not want_volumes:
            check(self.lib.molar_hip_sasa_frames(self.ctx, fa, F, natoms * 3, natoms, ia, n, va, C.c_float(probe), npoints, aa,
                                                 totals.ctypes.data))
            return areas, totals
        volumes, vtotals = per_atom(), np.zeros(F, np.float64)
        oa, k5 = _addr(volumes)
        check(self.lib.molar_hip_sasa_vol_frames(self.ctx, fa, F, natoms * 3, natoms, ia, n, va, C.c_float(probe), npoints, aa,
                                                 totals.ctypes.data, oa, vtotals.ctypes.data))
        return areas, totals, volumes, vtotals

    # ------------------------------------------------------------ measure
    def _sel_args(self, xyz, idx):
        xyz = _f32(xyz); idx = _u64(idx)
        xa, k1 = _addr(xyz); ia, k2 = _addr(idx)
        natoms = xyz.shape[0] if xyz.ndim == 2 else xyz.shape[0] // 3
        n = 0 if idx is None else idx.shape[0]
        return xa, natoms, ia, n, (k1, k2)

    @staticmethod
    def _box9(box):
        if box is None:
            return None, None
        b9 = box.colmajor9() if isinstance(box, PeriodicBox) else np.ascontiguousarray(
            np.asarray(box, np.float32).reshape(3, 3).T).reshape(9)
        return b9.ctypes.data, b9

    def min_max(self, xyz, idx=None):
        xa, na, ia, n, k = self._sel_args(xyz, idx)
        lo = np.zeros(3, np.float32); up = np.zeros(3, np.float32)
        check(self.lib.molar_hip_min_max(self.ctx, xa, na, ia, n, lo.ctypes.data, up.ctypes.data))
        return lo, up

    def center_of_geometry(self, xyz, idx=None):
        xa, na, ia, n, k = self._sel_args(xyz, idx)
        out = np.zeros(3, np.float32)
        check(self.lib.molar_hip_center_of_geometry(self.ctx, xa, na, ia, n, out.ctypes.data))
        return out

    def center_of_mass(self, xyz, mass, idx=None):
        xa, na, ia, n, k = self._sel_args(xyz, idx)
        mass = _f32(mass); ma, km = _addr(mass)
        out = np.zeros(3, np.float32)
        check(self.lib.molar_hip_center_of_mass(self.ctx, xa, na, ia, n, ma, out.ctypes.data))
        return out

    def center_of_geometry_pbc(self, xyz, box, dims=PBC_FULL, idx=None):
        xa, na, ia, n, k = self._sel_args(xyz, idx)
        ba, kb = self._box9(box)
        out = np.zeros(3, np.float32)
        check(self.lib.molar_hip_center_of_geometry_pbc(self.ctx, xa, na, ia, n, ba, pbc_mask(dims), out.ctypes.data))
        return out

    def center_of_mass_pbc(self, xyz, mass, box, dims=PBC_FULL, idx=None):
        xa, na, ia, n, k = self._sel_args(xyz, idx)
        mass = _f32(mass); ma, km = _addr(mass)
        ba, kb = self._box9(box)
        out = np.zeros(3, np.float32)
        check(self.lib.molar_hip_center_of_mass_pbc(self.ctx, xa, na, ia, n, ma, ba, pbc_mask(dims), out.ctypes.data))
        return out

    def gyration(self, xyz, mass, idx=None, box=None):
        xa, na, ia, n, k = self._sel_args(xyz, idx)
        mass = _f32(mass); ma, km = _addr(mass)
        ba, kb = self._box9(box)
        out = C.c_float(0)
        check(self.lib.molar_hip_gyration(self.ctx, xa, na, ia, n, ma, ba, C.byref(out)))
        return float(out.value)

    def inertia(self, xyz, mass, idx=None, box=None):
        """(moments[3] ascending, axes 3x3 with axes as columns, raw tensor 3x3)."""
        xa, na, ia, n, k = self._sel_args(xyz, idx)
        mass = _f32(mass); ma, km = _addr(mass)
        ba, kb = self._box9(box)
        mom = np.zeros(3, np.float32); axes = np.zeros(9, np.float32); tens = np.zeros(9, np.float32)
        check(self.lib.molar_hip_inertia(self.ctx, xa, na, ia, n, ma, ba, mom.ctypes.data, axes.ctypes.data,
                                         tens.ctypes.data))
        return mom, axes.reshape(3, 3).T.copy(), tens.reshape(3, 3).T.copy()

    def rmsd(self, xyz1, xyz2, idx1=None, idx2=None):
        a1 = self._sel_args(xyz1, idx1); a2 = self._sel_args(xyz2, idx2)
        out = C.c_float(0)
        check(self.lib.molar_hip_rmsd(self.ctx, *a1[:4], *a2[:4], C.byref(out)))
        return float(out.value)

    def rmsd_mw(self, xyz1, mass1, xyz2, idx1=None, idx2=None):
        a1 = self._sel_args(xyz1, idx1); a2 = self._sel_args(xyz2, idx2)
        mass1 = _f32(mass1); ma, km = _addr(mass1)
        out = C.c_float(0)
        check(self.lib.molar_hip_rmsd_mw(self.ctx, *a1[:4], ma, *a2[:4], C.byref(out)))
        return float(out.value)

    def fit_transform(self, xyz1, mass1, xyz2, mass2, idx1=None, idx2=None, at_origin=False):
        """(R, t) with p -> R @ p + t  (IsometryMatrix3, measure.rs:507-535)."""
        a1 = self._sel_args(xyz1, idx1); a2 = self._sel_args(xyz2, idx2)
        mass1 = _f32(mass1); m1, k1 = _addr(mass1)
        mass2 = _f32(mass2); m2, k2 = _addr(mass2)
        R = np.zeros(9, np.float32); t = np.zeros(3, np.float32)
        check(self.lib.molar_hip_fit_transform(self.ctx, *a1[:4], m1, *a2[:4], m2, 1 if at_origin else 0,
                                               R.ctypes.data, t.ctypes.data))
        return R.reshape(3, 3).T.copy(), t

    def apply_transform(self, xyz, R, t, idx=None):
        """In place on xyz (numpy float32 C-contiguous array or torch CUDA tensor)."""
        if not _is_torch(xyz):
            assert xyz.dtype == np.float32 and xyz.flags.c_contiguous, "apply_transform works in place"
        xa, na, ia, n, k = self._sel_args(xyz, idx)
        Rf = np.ascontiguousarray(np.asarray(R, np.float32).T).reshape(9)
        tf = np.ascontiguousarray(t, np.float32)
        check(self.lib.molar_hip_apply_transform(self.ctx, xa, na, ia, n, Rf.ctypes.data, tf.ctypes.data))
        return xyz

    def unwrap_simple(self, xyz, box, dims=PBC_FULL, idx=None):
        if not _is_torch(xyz):
            assert xyz.dtype == np.float32 and xyz.flags.c_contiguous, "unwrap_simple works in place"
        xa, na, ia, n, k = self._sel_args(xyz, idx)
        ba, kb = self._box9(box)
        check(self.lib.molar_hip_unwrap_simple(self.ctx, xa, na, ia, n, ba, pbc_mask(dims)))
        return xyz

    def unwrap_connectivity(self, xyz, box, cutoff, dims=PBC_FULL, idx=None):
        """Modify::unwrap_connectivity_dim (modify.rs:72-131) in place: GPU neighbour search with local ids, adjacency in
        pair order and the reference's stack walk inside the library (molar_hip_unwrap_connectivity).  Returns the list of
        groups of LOCAL indices the reference returns as selections."""
        if not _is_torch(xyz):
            assert xyz.dtype == np.float32 and xyz.flags.c_contiguous, "unwrap_connectivity works in place"
        if idx is not None and len(idx) == 0:      # (a NULL index means "all atoms" to the C ABI: never pass an empty one as NULL)
            raise ValueError("unwrap_connectivity: empty selection")
        xa, na, ia, n, k = self._sel_args(xyz, idx)
        nsel = n if idx is not None else na
        ba, kb = self._box9(box)
        goff = np.zeros(nsel + 1, np.uint64); gids = np.zeros(max(nsel, 1), np.uint64)
        ng = C.c_size_t(0)
        check(self.lib.molar_hip_unwrap_connectivity(self.ctx, xa, na, ia, n, ba, float(cutoff), pbc_mask(dims), goff.ctypes.data,
                                                     gids.ctypes.data, C.byref(ng)))
        return [gids[int(goff[g]):int(goff[g + 1])].copy() for g in range(int(ng.value))]

    def center_batch(self, xyz, idx, offsets, mass=None):
        """Centres of K selections given as CSR (idx, offsets[K+1]): center_of_mass if `mass` is given,
        else center_of_geometry.  One wave per selection; returns float32 [K,3]."""
        xyz = _f32(xyz); idx = _u64(idx); offsets = _u64(offsets); mass = _f32(mass)
        xa, k1 = _addr(xyz); ia, k2 = _addr(idx); oa, k3 = _addr(offsets); ma, k4 = _addr(mass)
        K = offsets.shape[0] - 1
        out = np.zeros((K, 3), np.float32)
        check(self.lib.molar_hip_center_batch(self.ctx, xa, xyz.shape[0], ia, oa, K, ma, out.ctypes.data))
        return out

    def unwrap_simple_batch(self, xyz, idx, offsets, box, dims=PBC_FULL):
        """unwrap_simple on each of K CSR selections, in place."""
        if not _is_torch(xyz):
            assert xyz.dtype == np.float32 and xyz.flags.c_contiguous
        idx = _u64(idx); offsets = _u64(offsets)
        xa, k1 = _addr(xyz); ia, k2 = _addr(idx); oa, k3 = _addr(offsets)
        ba, kb = self._box9(box)
        check(self.lib.molar_hip_unwrap_simple_batch(self.ctx, xa, xyz.shape[0], ia, oa, offsets.shape[0] - 1, ba,
                                                     pbc_mask(dims)))
        return xyz

    def lipid_tail_order_csr(self, xyz, idx, tail_offsets, order_type, normals, normal_offsets, bond_orders):
        """Same as lipid_tail_order with the CSR arrays prepared by the caller (no per-call Python loops)."""
        xyz = _f32(xyz)
        xa, kx = _addr(xyz)
        idx = _u64(idx); tail_offsets = np.ascontiguousarray(tail_offsets, np.uint64)
        normal_offsets = np.ascontiguousarray(normal_offsets, np.uint64)
        normals = np.ascontiguousarray(normals, np.float32)
        if not _is_torch(bond_orders):                      # idx and bond_orders may live on the GPU (torch int64 / uint8)
            bond_orders = np.ascontiguousarray(bond_orders, np.uint8)
        ia, ki = _addr(idx); ba, kb = _addr(bond_orders)
        K = len(tail_offsets) - 1
        nout = int(tail_offsets[-1]) - 2 * K
        out = np.zeros(max(nout, 1), np.float32)
        check(self.lib.molar_hip_lipid_tail_order(self.ctx, xa, xyz.shape[0], ia, tail_offsets.ctypes.data, K,
                                                  int(order_type), normals.ctypes.data, normal_offsets.ctypes.data,
                                                  ba, out.ctypes.data))
        return out[:nout]

    def copy_bandwidth(self, nbytes=1 << 30, reps=10) -> float:
        """Measured device-to-device copy rate in GB/s (read + write), best of the library's float4 copy kernels."""
        out = C.c_float(0)
        check(self.lib.molar_hip_copy_bandwidth(self.ctx, int(nbytes), int(reps), C.byref(out)))
        return float(out.value)

    def write_bandwidth(self, nbytes=1 << 30, reps=10) -> float:
        """Measured write-only float4 stream rate in GB/s."""
        out = C.c_float(0)
        check(self.lib.molar_hip_write_bandwidth(self.ctx, int(nbytes), int(reps), C.byref(out)))
        return float(out.value)

    def membrane_smooth(self, box, state, patch_offsets, patch_ids):
        """One iteration of Membrane::smooth (molar_membrane/src/lib.rs:661-812) on the GPU.  `state` is a dict of
        per-lipid arrays updated IN PLACE (see new_membrane_state); a lipid that turns invalid keeps its old
        values, like the fields of the reference's LipidMolecule."""
        pb = box if isinstance(box, PeriodicBox) else PeriodicBox.from_matrix(box)
        if state["head_markers"].dtype != np.float32:
            raise TypeError("Engine.membrane_smooth takes a float32 state; MeasureF64.membrane_smooth the float64 one")
        m9 = pb.colmajor9()
        return _membrane_smooth_call(self.lib.molar_hip_membrane_smooth, self.ctx, m9.ctypes.data, state, patch_offsets,
                                     patch_ids, np.float32)

    def lipid_tail_order(self, xyz, tails, order_type, normals, bond_orders):
        """Batched Measure::lipid_tail_order (measure.rs:270-422).  tails: list of index arrays (the
        tail carbons, in chain order); normals: list of [1,3] or [n-2,3] arrays; bond_orders: list of
        n-1 arrays of 1/2.  order_type: 0 Sz, 1 Scd, 2 ScdCorr.  Returns a list of n-2 arrays."""
        xyz = _f32(xyz)
        xa, kx = _addr(xyz)
        natoms = xyz.shape[0]
        lens = np.array([len(t) for t in tails], dtype=np.uint64)
        toff = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        idx = np.ascontiguousarray(np.concatenate([np.asarray(t, np.uint64) for t in tails]))
        nl = [np.asarray(n, np.float32).reshape(-1, 3) for n in normals]
        noff = np.concatenate([[0], np.cumsum([len(n) for n in nl])]).astype(np.uint64)
        nrm = np.ascontiguousarray(np.concatenate(nl))
        bo = np.ascontiguousarray(np.concatenate([np.asarray(b, np.uint8) for b in bond_orders])) if bond_orders is not None else None
        if bo is not None and len(bo) != int(toff[-1]) - len(tails):
            raise MolarHipError(9, "for N tail carbons # of bond orders should be N-1")       # LipidOrderError::BondOrderCount
        nout = max(int(toff[-1]) - 2 * len(tails), 0)
        out = np.zeros(max(nout, 1), np.float32)
        check(self.lib.molar_hip_lipid_tail_order(self.ctx, xa, natoms, idx.ctypes.data, toff.ctypes.data, len(tails),
                                                  int(order_type), nrm.ctypes.data, noff.ctypes.data,
                                                  None if bo is None else bo.ctypes.data, out.ctypes.data))
        res, pos = [], 0
        for n in lens:
            res.append(out[pos:pos + int(n) - 2].copy())
            pos += int(n) - 2
        return res

    # ------------------------------------------------------------ CSR-batched Measure (ParSplit-style loops)
    def gyration_batch(self, xyz, idx, offsets, mass, box=None):
        """Measure::gyration (measure.rs:78-87; gyration_pbc :222-232 with a box) of each of the K selections
        idx[offsets[k]:offsets[k+1]] - what MolAR runs from rayon over a ParSplit (system.rs:193-213)."""
        xyz = _f32(xyz); idx = _u64(idx); offsets = _u64(offsets); mass = _f32(mass)
        xa, k1 = _addr(xyz); ia, k2 = _addr(idx); oa, k3 = _addr(offsets); ma, k4 = _addr(mass)
        ba, kb = self._box9(box)
        K = len(offsets) - 1
        out = np.zeros(max(K, 1), np.float32)
        check(self.lib.molar_hip_gyration_batch(self.ctx, xa, xyz.shape[0], ia, oa, K, ma, ba, out.ctypes.data))
        return out[:K]

    def rmsd_batch(self, xyz1, xyz2, idx, offsets, mass=None, idx2=None):
        """rmsd (measure.rs:485-504; rmsd_mw :538-558 with `mass`) of selection k in frame 1 against selection k in frame 2."""
        xyz1 = _f32(xyz1); xyz2 = _f32(xyz2); idx = _u64(idx); idx2 = _u64(idx2); offsets = _u64(offsets); mass = _f32(mass)
        a1, k1 = _addr(xyz1); a2, k2 = _addr(xyz2); ia, k3 = _addr(idx); ja, k4 = _addr(idx2); oa, k5 = _addr(offsets)
        ma, k6 = _addr(mass)
        K = len(offsets) - 1
        out = np.zeros(max(K, 1), np.float32)
        check(self.lib.molar_hip_rmsd_batch(self.ctx, a1, xyz1.shape[0], ia, a2, xyz2.shape[0], ja, oa, K, ma, out.ctypes.data))
        return out[:K]

    def fit_batch(self, xyz1, mass1, xyz2, idx, offsets, idx2=None, mass2=None, apply=False):
        """fit_transform (measure.rs:507-522) of each selection of frame 1 onto its counterpart in frame 2; `apply`
        moves the selections of xyz1 in place.  mass2=None (or mass1 itself): one mass column, read through idx2 for the
        second selection's centre (MolarHipError 50 if idx2 differs from idx and frame 2 has more atoms than that column).
        Returns dict(R[K,3,3], t[K,3], rmsd[K], com[K,3], gyration[K]); the last three describe the fitted selections."""
        if apply and not _is_torch(xyz1):
            assert xyz1.dtype == np.float32 and xyz1.flags.c_contiguous, "apply works in place"
        xyz1 = _f32(xyz1); xyz2 = _f32(xyz2); idx = _u64(idx); idx2 = _u64(idx2); offsets = _u64(offsets)
        mass1 = _f32(mass1); mass2 = _f32(mass2)
        a1, k1 = _addr(xyz1); a2, k2 = _addr(xyz2); ia, k3 = _addr(idx); ja, k4 = _addr(idx2); oa, k5 = _addr(offsets)
        m1, k6 = _addr(mass1); m2, k7 = _addr(mass2)
        K = len(offsets) - 1
        R = np.zeros((max(K, 1), 9), np.float32); t = np.zeros((max(K, 1), 3), np.float32)
        rm = np.zeros(max(K, 1), np.float32); com = np.zeros((max(K, 1), 3), np.float32); gy = np.zeros(max(K, 1), np.float32)
        check(self.lib.molar_hip_fit_batch(self.ctx, a1, xyz1.shape[0], ia, m1, a2, xyz2.shape[0], ja, m2, oa, K,
                                           1 if apply else 0, R.ctypes.data, t.ctypes.data, rm.ctypes.data,
                                           com.ctypes.data, gy.ctypes.data))
        return dict(R=R[:K].reshape(K, 3, 3).transpose(0, 2, 1).copy(), t=t[:K], rmsd=rm[:K], com=com[:K], gyration=gy[:K])

    def translate(self, xyz, shift, idx=None):
        """Modify::translate (modify.rs:16-23), in place."""
        if not _is_torch(xyz):
            assert xyz.dtype == np.float32 and xyz.flags.c_contiguous, "translate works in place"
        xa, na, ia, n, k = self._sel_args(xyz, idx)
        sh = np.ascontiguousarray(shift, np.float32).reshape(3)
        check(self.lib.molar_hip_translate(self.ctx, xa, na, ia, n, sh.ctypes.data))
        return xyz

    def rotate(self, xyz, unit_axis, angle, idx=None):
        """Modify::rotate (modify.rs:25-30): Rotation3::from_axis_angle about the origin, in place."""
        if not _is_torch(xyz):
            assert xyz.dtype == np.float32 and xyz.flags.c_contiguous, "rotate works in place"
        xa, na, ia, n, k = self._sel_args(xyz, idx)
        ax = np.ascontiguousarray(unit_axis, np.float32).reshape(3)
        check(self.lib.molar_hip_rotate(self.ctx, xa, na, ia, n, ax.ctypes.data, float(angle)))
        return xyz

    def principal_transform(self, xyz, mass, idx=None, box=None):
        """Measure::principal_transform (measure.rs:102-109; _pbc :246-257 with a box) as (R[3,3], t[3]), p -> R p + t."""
        xa, na, ia, n, k = self._sel_args(xyz, idx)
        mass = _f32(mass); ma, km = _addr(mass)
        ba, kb = self._box9(box)
        R = np.zeros(9, np.float32); t = np.zeros(3, np.float32)
        check(self.lib.molar_hip_principal_transform(self.ctx, xa, na, ia, n, ma, ba, R.ctypes.data, t.ctypes.data))
        return R.reshape(3, 3).T.copy(), t

    def fit_rmsd_batch(self, frames, mass, ref_xyz, idx=None, ref_idx=None, apply=True):
        """frames: [F, natoms, 3] (numpy, modified in place if apply; or torch CUDA tensor).
        Returns dict(rmsd[F], R[F,3,3], t[F,3], com[F,3], gyration[F])."""
        if _is_torch(frames):
            F, natoms = frames.shape[0], frames.shape[1]
            fa, kf = _addr(frames.contiguous())
        else:
            assert frames.dtype == np.float32 and frames.flags.c_contiguous
            F, natoms = frames.shape[0], frames.shape[1]
            fa, kf = _addr(frames)
        idx = _u64(idx); ref_idx = _u64(ref_idx) if ref_idx is not None else idx
        ia, ki = _addr(idx); ra, kr = _addr(ref_idx)
        n = 0 if idx is None else idx.shape[0]
        mass = _f32(mass); ma, km = _addr(mass)
        ref_xyz = _f32(ref_xyz); xa, kx = _addr(ref_xyz)
        ref_natoms = ref_xyz.shape[0] if ref_xyz.ndim == 2 else ref_xyz.shape[0] // 3
        rm = np.zeros(F, np.float32); R = np.zeros((F, 9), np.float32); t = np.zeros((F, 3), np.float32)
        com = np.zeros((F, 3), np.float32); gy = np.zeros(F, np.float32)
        check(self.lib.molar_hip_fit_rmsd_batch(self.ctx, fa, F, natoms, ia, n, ma, xa, ref_natoms, ra,
                                                1 if apply else 0, rm.ctypes.data, R.ctypes.data, t.ctypes.data,
                                                com.ctypes.data, gy.ctypes.data))
        return dict(rmsd=rm, R=R.reshape(F, 3, 3).transpose(0, 2, 1).copy(), t=t, com=com, gyration=gy)

    def rmsd_matrix(self, frames, idx=None, mass=None, frames2=None, fit=True, out=None):
        """All-pairs minimum RMSD (molar_hip_rmsd_matrix): frames [F, natoms, 3] float32, numpy or torch CUDA (rows may be
        strided: frames[::2] or a wider last-but-one stride are read in place).  out[a][b] = mass-weighted RMSD of frame a
        fitted onto frame b (`mass`: one per atom, None: unit weights; `idx`: the selection, None: every atom; fit=False: no
        superposition).  frames2=None: the symmetric [F, F] matrix, exactly symmetric with a zero diagonal; otherwise
        [F, F2] of `frames` against `frames2`.  numpy in, numpy out; torch CUDA in, torch CUDA out, written on the ENGINE's
        stream and not waited for: `Engine.synchronize()` before torch reads it (the call waits for torch's current stream
        first, and for its own kernels only when it had to copy an argument to make it contiguous).
        `out`: an optional [F, >= columns] destination of the same kind."""
        return _rmsd_matrix_call(self.lib, self.lib.molar_hip_rmsd_matrix, self.ctx, frames, idx, mass, frames2, fit, out, np.float32)

    def fluctuations(self, frames, idx=None, mass=None, ref=None, fit=True, iterations=0, cov=False, fit_out=False, out=None):
        """Mean structure, per-atom RMSF and (cov=True) the 3n x 3n positional covariance of frames [F, natoms, 3] float32 about
        their mean, after the mass-weighted fit of every frame onto `ref` ([n, 3], the selected atoms; None: frame 0) - with
        iterations=I the mean of a pass becomes the reference of the next, 1 + I passes (molar_hip_fluct; the definition:
        molar_hip.h).  `mass`: one per atom, None: unit weights; `idx`: the selection, None: every atom; fit=False: the frames
        as they stand.  Statistics are unweighted, two-pass and formed in float64.  fit_out=True also returns, per frame,
        R (9, column-major), t (3) and the weighted RMSD to the reference of the last pass.  Returns
        Fluctuations(mean [n, 3], rmsf [n], cov [3n, 3n] or None, fit [F, 13] or None): numpy in, numpy out; torch CUDA in,
        torch CUDA out, written on the ENGINE's stream and not waited for (`Engine.synchronize()` before torch reads them).
        `out`: an optional Fluctuations (or 4-tuple) of destinations of the same kind; None entries are allocated."""
        return _fluct_call(self.lib, self.lib.molar_hip_fluct, self.ctx, frames, idx, mass, ref, fit, iterations, cov, fit_out, out, np.float32)

    def msd(self, frames, idx=None, mass=None, boxes=None, pbc=7, groups=None, ref_idx=None, max_lag=None, origin_stride=1, dims=7,
            m4=True, per_particle=False, disp=False, msd=True, out=None):
        """Mean-squared displacement over all time origins of frames [F, natoms, 3] float32 (molar_hip_msd; the definition:
        molar_hip.h).  Every selected atom (`idx`, None: every atom) is followed from frame to frame with the periodic jumps
        removed (`boxes`: one column-major box [9] or [3, 3] transposed into it, or one per frame [F, 9]; None: the
        trajectory is already unwrapped; `pbc`: the PbcDims byte, see pbc_mask).  `groups`: CSR offsets [P + 1] over the
        selection order, each group a particle followed by its centre of mass (`mass`: one per atom, None: unit weights);
        None: every selected atom is a particle.  `ref_idx`: a second selection whose weighted mean displacement (the drift)
        is subtracted.  Lags 0 .. max_lag (None: F - 1), origins 0, origin_stride, ...; `dims`: the bits x, y, z of the
        components that enter.  Returns Msd(msd [L + 1], m4 [L + 1], msd_particle [P, L + 1], disp [F, P, 3]); the entries
        not asked for (msd=, m4=, per_particle=, disp=) are None.  numpy in, numpy out; torch CUDA in, torch CUDA out, written
        on the ENGINE's stream and not waited for (`Engine.synchronize()` before torch reads them).  `out`: an optional Msd
        (or 4-tuple) of destinations of the same kind; None entries are allocated."""
        return _msd_call(self.lib, self.lib.molar_hip_msd, self.ctx, frames, idx, mass, boxes, pbc, groups, ref_idx, max_lag, origin_stride, dims,
                         msd, m4, per_particle, disp, out, np.float32)

    def internal_coords(self, frames, tuples, kind=None, labels=None, ngroups=None, boxes=None, pbc=7, nbins=0, range=None, pairs=None,
                        pair_labels=None, npair_groups=None, map_bins=0, want=None, out=None):
        """Distances, angles or dihedrals of `tuples` [T, 2 | 3 | 4] (atom indices; kind: from tuples.shape[1]) in every frame of
        frames [F, natoms, 3] float32 (molar_hip_intcoord, the definition: molar_hip.h), radians, all arithmetic in double.
        Every bond vector takes the minimum image under `boxes` ([9] column-major, [3, 3] rows or [F, 9]; None: no image is
        removed) on the dimensions of `pbc`.  Returns InternalCoords(values [F, T] (NaN where invalid), hist [G, nbins] per
        group of `labels` (one per tuple), map [G2, map_bins, map_bins]: the joint histogram of the two tuples of every row of
        `pairs` [P, 2] per group of `pair_labels` (the Ramachandran map), mean [T], spread [T] (the standard deviation; the
        circular variance for dihedrals, see circular_std), valid [T]: the frames that entered, edges: the bin edges of hist,
        or of one side of the map without one).  Distances are binned in the half-open `range` = (lo, hi).  `want`: the names to
        compute (default: all that the arguments allow); numpy in gives numpy out, torch CUDA in gives torch CUDA out
        (integers as int64).  `out`: an optional InternalCoords (or 6-tuple) of destinations; values may have a row stride
        above T.  The same call gives the same bits."""
        return _intcoord_call(self.lib, self.lib.molar_hip_intcoord, self.ctx, frames, tuples, kind, labels, ngroups, boxes, pbc, nbins, range, pairs,
                              pair_labels, npair_groups, map_bins, want, out, np.float32)

    def vector_correlations(self, frames, tuples, kind=None, labels=None, ngroups=None, boxes=None, pbc=7, mode="unit", dims=7, max_lag=None,
                            origin_stride=1, want=None, out=None):
        """Time correlation functions over all time origins of the vectors of `tuples` [V, 1 | 2 | 3] (atom indices; kind: from
        tuples.shape[1]; a 1-D array is kind 1) in frames [F, natoms, 3] float32 (molar_hip_tcf, the definition:
        molar_hip.h), all arithmetic in double.  Kind 1: the atom's own 3-vector (a block of velocities, dipoles or
        angle_vectors); kind 2: the bond vector B - A; kind 3: the plane normal (B - A) x (C - A); bonds take the minimum image
        under `boxes` ([9] column-major, [3, 3] rows or [F, 9]; None: no image is removed) on the dimensions of `pbc`.
        mode "unit": unit vectors, "raw": the vectors as they are (c2, c2_vec and s2 are defined for "unit" only); `dims`: the
        bits x, y, z of the components that enter.  Lags 0 .. max_lag (None: F - 1), origins 0, origin_stride, ...  Returns
        VectorCorrelations(c1 [G, L + 1], c2 [G, L + 1] per group of `labels` (one per vector), c1_vec [V, L + 1],
        c2_vec [V, L + 1], nvalid [G], mean [V, 3], s2 [V], bad_frames [V], lags: n(tau)); a vector with a bad frame (a
        component that is not finite, zero length in "unit" mode) is left out of every sum and is NaN in its own rows.
        `want`: the names to compute (default: c1, c2, nvalid, mean, s2, bad_frames - those the mode allows); numpy in
        gives numpy out, torch CUDA in gives torch CUDA out (nvalid as int64, bad_frames as int32), written on the ENGINE's
        stream and not waited for.  `out`: an optional VectorCorrelations (or 8-tuple) of destinations; c1_vec and c2_vec may
        share a row stride above L + 1.  The same call gives the same bits."""
        return _tcf_call(self.lib, self.lib.molar_hip_tcf, self.ctx, frames, tuples, kind, labels, ngroups, boxes, pbc, mode, dims, max_lag,
                         origin_stride, want, out, np.float32)

    def density(self, frames, grid, idx=None, weight=None, labels=None, ngroups=None, boxes=None, pbc=7, centre_idx=None,
                centre_weight=None, want=None, out=None):
        """Density profiles and maps of frames [F, natoms, 3] float32 over `grid` (profile_grid, map_grid, volume_grid;
        molar_hip_density, the definition: molar_hip.h): the mean over the frames of the sum of `weight` (one per ATOM: masses,
        charges, electron counts; None: number density) per unit volume in every bin, per group of `labels` (one per SELECTED
        atom, below `ngroups`; None: one group).  `boxes`: [9] column-major, [3, 3] rows, or [F, 9], needed by the fractional
        grids; `pbc`: the periodic dimensions, wrapped.  `centre_idx` / `centre_weight` (per ATOM): the set a centred grid is
        centred on in every frame.  Returns Density(density [G, nx, ny, nz], count (uint64; torch: int64), outside [F],
        centre [F, 3], binvol [F], weight_scale_log2, grid); with `want` (a tuple of those names) the others are None.  numpy in, numpy out;
        torch CUDA in, torch CUDA out, written on the ENGINE's stream and not waited for (`Engine.synchronize()` before torch
        reads them).  `out`: an optional Density (or 5-tuple) of destinations.  The same call gives the same bits."""
        return _density_call(self.lib, self.lib.molar_hip_density, self.ctx, frames, grid, idx, weight, labels, ngroups, boxes, pbc, centre_idx,
                             centre_weight, want, out, np.float32)

    def structure_factor(self, frames, grid, idx=None, weight=None, labels=None, ngroups=None, boxes=None, want=None, out=None):
        """Static structure factors of frames [F, natoms, 3] float32 by the direct sum over the reciprocal lattice of `boxes`
        ([9] column-major, [3, 3] rows, or [F, 9]: the frame's box, or any fixed matrix for a fixed q grid) up to the Miller
        indices of `grid` (sfactor_grid; molar_hip_sfactor, the definition: molar_hip.h), all arithmetic in double on the f64
        matrix cores.  `weight`: one per ATOM, of any sign (scattering lengths, electron counts; None: 1); `labels`: one per
        SELECTED atom, below `ngroups`, the species (None: one group).  Returns StructureFactor(rho [F, G, Q, 2]: the
        collective density (re, im) of every group at every lattice point, h >= 0 only (sfactor_miller); frame_ok [F]: 0 where
        a selected coordinate is not finite - that frame is NaN in rho and enters no average; rho_mean [G, Q, 2]: its mean over
        the ok frames; sab [P, Q]: the mean of Re(rho_a conj rho_b) over the ok frames for the pairs a <= b, a-major, not
        normalised (sfactor_normalize); shell [P, nshells], shell_count [nshells]: the average over the lattice points of
        each shell of |q| (sfactor_shell_centres), |q| from each frame's own box; grid).  `want`: the names to compute
        (default: frame_ok, sab, and shell, shell_count when the grid has shells); numpy in gives numpy out, torch CUDA in
        gives torch CUDA out (frame_ok as int32, shell_count as int64), written on the ENGINE's stream and not waited for.
        `out`: an optional StructureFactor (or 6-tuple) of destinations; rho may have a row stride above 2 Q (a wider last but
        one dimension sliced).  The same call gives the same bits."""
        return _sfactor_call(self.lib, self.lib.molar_hip_sfactor, self.ctx, frames, grid, idx, weight, labels, ngroups, boxes, want, out, np.float32)

    def min_distances(self, frames, idx1=None, idx2=None, labels1=None, labels2=None, ngroups1=None, ngroups2=None, boxes=None, pbc=7, same=False,
                      exclude_same_group=False, cutoff=0.0, frame_block=0, want=None, out=None, n1=None, n2=None):
        """Minimum distances between two selections of frames [F, natoms, 3] float32 (molar_hip_mindist, the definition:
        molar_hip.h): every pair is evaluated under the minimum image of each frame's own box (`boxes` [9] column-major,
        [3, 3] rows or [F, 9]; None: plain differences; `pbc`: the PbcDims mask), in double.  Set 1 is `idx1` (None: atoms
        0 .. n1 - 1, n1 = natoms by default), set 2 `idx2`; `same=True`: set 2 is set 1, the pair i = i is skipped, and with
        `exclude_same_group` every pair inside one group.  `labels1` / `labels2`: one label per SELECTED atom, below
        `ngroups1` / `ngroups2`: residues, lipids, molecules (mindist_groups_from_resindex).  Returns MinDistances(dist [F],
        pair [F, 2]: the smallest distance of the frame and the positions (i, j) within the sets that have it, the lowest (i, j)
        among equal distances; atom1 [F, n1], near1 [F, n1]: for every atom of set 1 its distance to set 2 and the position
        of its nearest atom there; atom2 [F, n2]: the distances seen from set 2; mat [F, G1, G2]: the smallest distance
        between every pair of groups; mat_mean (float64), mat_min, mat_freq [G1, G2]: its mean, its minimum and the number of
        frames below `cutoff` over the valid frames; frame_ok [F]: 0 where a selected coordinate is not finite or the box is
        refused - that frame is NaN (pair, near1: the largest uint64, -1 as int64) and enters no reduction; nvalid [1]).
        `want`: the names to compute (default: dist, pair, frame_ok, nvalid); numpy in gives numpy out, torch CUDA in gives
        torch CUDA out (pair, near1, nvalid as int64, mat_freq, frame_ok as int32), written on the ENGINE's stream and not
        waited for.  `out`: an optional MinDistances (or 11-tuple) of destinations; atom1, near1 and atom2 may have a row
        stride (a wider last dimension sliced; atom1 and near1 the same one).  Only minima under a total order and sums in
        frame order: the same call gives the same bits, whatever `frame_block` is."""
        return _mindist_call(self.lib, self.lib.molar_hip_mindist, self.ctx, frames, idx1, idx2, labels1, labels2, ngroups1, ngroups2, boxes, pbc, same,
                             exclude_same_group, cutoff, frame_block, want, out, n1, n2, np.float32)

    def van_hove(self, traj, lags, range, nbins, idx=None, labels=None, ngroups=None, origin_stride=1, dims=7, signed=False, want=None, out=None):
        """The self part of the van Hove function of an ALREADY UNWRAPPED particle trajectory traj [F, natoms, 3] float32 - the
        `disp` of msd(), or raw coordinates of a system that is not periodic (molar_hip_vanhove, the definition: molar_hip.h):
        for every lag of the list `lags` (strictly increasing, below F, 0 allowed; vanhove_lags) and every origin 0,
        origin_stride, ... the displacement sqrt(sum of the squared components of `dims`) of every selected particle (`idx`,
        None: all), or with signed=True the one component itself, counted into `nbins` bins of the half-open `range` =
        (lo, hi) per group of `labels` (one per SELECTED particle, below `ngroups`; None: one group), all in double.  No box is
        taken and no image removed: that is msd's work (van_hove_frames chains the two).  Returns VanHove(hist [G, L, nbins],
        outside [G, L]: the pairs beyond the range, norigins [L], nvalid [G]: the particles that entered, bad [n]: the frames
        with a coordinate that is not finite, per particle - such a particle enters no count -, edges [nbins + 1]).  For
        every (g, l): hist.sum(-1) + outside == nvalid[g] * norigins[l].  `want`: the names to compute (default: all);
        numpy in gives numpy out (uint64, bad uint32), torch CUDA in gives torch CUDA out (int64, bad int32), written on the
        ENGINE's stream and not waited for.  `out`: an optional VanHove (or 5-tuple) of destinations.  Every result is an
        integer: the same call gives the same bits.  vanhove_density and vanhove_fs turn the counts into G_s and F_s(q, tau)."""
        return _vanhove_call(self.lib, self.lib.molar_hip_vanhove, self.ctx, traj, lags, range, nbins, idx, labels, ngroups, origin_stride, dims, signed,
                             want, out, np.float32)

    def van_hove_frames(self, frames, lags, range, nbins, idx=None, boxes=None, pbc=7, mass=None, groups=None, ref_idx=None, labels=None, ngroups=None,
                        origin_stride=1, dims=7, signed=False, want=None, out=None):
        """van_hove of WRAPPED frames [F, natoms, 3] float32: msd(frames, idx, mass, boxes, pbc, groups, ref_idx, disp=True,
        msd=False, m4=False) makes the unwrapped particle trajectory (no-jump unwrap under `boxes`, centres of mass of the CSR
        `groups`, the drift of `ref_idx` removed), then van_hove runs on that `disp` with `labels` one per PARTICLE (per group
        of `groups`, or per selected atom without them).  With torch CUDA frames `disp` stays on the device between the two
        calls; with numpy frames it makes one extra round trip through host memory.  Returns the VanHove of van_hove."""
        return _vanhove_frames_call(self.msd, self.van_hove, frames, lags, range, nbins, idx, mass, boxes, pbc, groups, ref_idx, labels, ngroups,
                                    origin_stride, dims, signed, want, out)


class FitStream:
    """molar_hip_fit_stream_*: the per-frame fit loop of benches/comparison_small.rs:14-25 for frames in HOST memory (numpy),
    three in flight - `t = fs.begin(frame_k1); out = fs.end(t_k)`.  The selected atoms are packed by host threads and only
    they cross the link; every record equals fit_rmsd_batch's for the same frame.  apply=True moves the selection inside the
    numpy frame handed to begin() (keep it alive and untouched until end())."""

    def __init__(self, engine: "Engine", natoms, mass, ref_xyz, idx=None, ref_idx=None, host_threads=0):
        self.eng, self.lib = engine, engine.lib
        idx = None if idx is None else np.ascontiguousarray(idx, np.uint64)
        ref_idx = idx if ref_idx is None else np.ascontiguousarray(ref_idx, np.uint64)
        mass = np.ascontiguousarray(mass, np.float32)
        ref_xyz = np.ascontiguousarray(ref_xyz, np.float32)
        self.natoms = int(natoms)
        h = C.c_void_p()
        check(self.lib.molar_hip_fit_stream_create(engine.ctx, self.natoms, None if idx is None else idx.ctypes.data,
                                                   0 if idx is None else len(idx), mass.ctypes.data, ref_xyz.ctypes.data,
                                                   ref_xyz.shape[0] if ref_xyz.ndim == 2 else ref_xyz.shape[0] // 3,
                                                   None if ref_idx is None else ref_idx.ctypes.data, int(host_threads), C.byref(h)))
        self.h = h
        self._frames = {}

    def begin(self, frame, apply=False) -> int:
        assert isinstance(frame, np.ndarray) and frame.dtype == np.float32 and frame.flags.c_contiguous and frame.size == self.natoms * 3
        t = C.c_int32(-1)
        check(self.lib.molar_hip_fit_stream_begin(self.h, frame.ctypes.data, 1 if apply else 0, C.byref(t)))
        self._frames[t.value] = frame
        return t.value

    def end(self, ticket):
        rm = C.c_float(); gy = C.c_float()
        R = np.zeros(9, np.float32); t = np.zeros(3, np.float32); com = np.zeros(3, np.float32)
        check(self.lib.molar_hip_fit_stream_end(self.h, ticket, C.byref(rm), R.ctypes.data, t.ctypes.data, com.ctypes.data, C.byref(gy)))
        self._frames.pop(ticket, None)
        return dict(rmsd=np.float32(rm.value), R=R.reshape(3, 3).T.copy(), t=t, com=com, gyration=np.float32(gy.value))

    def close(self):
        if self.h:
            self.lib.molar_hip_fit_stream_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Contacts:
    """Result of a contacts call: `count` (entries of the pair list, None when not asked for), `deg1` / `deg2` (per
    selected atom; deg2 is None for a single-set search, whose deg1 counts both members), `map` (group x group, upper
    triangle for a single-set search) and, from the frames form, `occupancy` (frames in which a group pair was in
    contact)."""

    def __init__(self, count, deg1, deg2, cmap, occupancy=None):
        self.count, self.deg1, self.deg2, self.map, self.occupancy = count, deg1, deg2, cmap, occupancy


class Clusters:
    """Connected components of a contact graph: `ncomponents` (C); `comp_of` [P], the component of each particle; `sizes` [C];
    `offsets` [C + 1] and `members` [P], the particles of component k at members[offsets[k] : offsets[k + 1]], ascending (None
    when the members were not asked for).  Components are numbered in the order of their smallest particle."""

    def __init__(self, ncomponents, comp_of, sizes, offsets, members):
        self.ncomponents, self.comp_of, self.sizes, self.offsets, self.members = ncomponents, comp_of, sizes, offsets, members

    def split(self):
        """The components as a list of index arrays (particle numbers, ascending), in the components' order."""
        if self.members is None:
            raise ValueError("Clusters.split: the call was made with want_members=False")
        off = self.offsets.cpu().numpy() if _is_torch(self.offsets) else np.asarray(self.offsets)
        mem = self.members.cpu().numpy() if _is_torch(self.members) else np.asarray(self.members)
        off = off.astype(np.int64)
        return [mem[off[k]:off[k + 1]].astype(np.int64) for k in range(self.ncomponents)]


class ClustersBlock:
    """Connected components over a block of frames: `ncomponents` and `largest` per frame, `size_hist` [P + 1] (components of
    each size, summed over the frames) and `comp_of` [nframes, P] (None when not asked for)."""

    def __init__(self, ncomponents, largest, size_hist, comp_of):
        self.ncomponents, self.largest, self.size_hist, self.comp_of = ncomponents, largest, size_hist, comp_of


HBOND_DHA_MIN, HBOND_HDA_MAX = 0, 1


class HBonds:
    """Hydrogen bonds of a frame: `count`; `triples` [count, 3] (donor, hydrogen, acceptor as atom indices of the frame, sorted by
    the donor's position in its selection, the hydrogen's position in the donors' CSR, the acceptor's position); the float64
    columns `dist_da`, `dist_ha`, `angle` (degrees; of the kind that was asked for); `don_count` / `acc_count` per selected donor /
    acceptor and `map` (donor group x acceptor group)."""

    def __init__(self, count, triples, dist_da, dist_ha, angle, don_count, acc_count, cmap):
        self.count, self.triples, self.dist_da, self.dist_ha, self.angle = count, triples, dist_da, dist_ha, angle
        self.don_count, self.acc_count, self.map = don_count, acc_count, cmap


class HBondsBlock:
    """Hydrogen bonds of a block of frames: `per_frame` counts; the lists of the frames one after the other (`triples` and the
    columns, frame f at frame_offsets[f] : frame_offsets[f + 1]); `table` [unique, 3] - the block's distinct bonds in the order
    of HBonds.triples - with `occupancy` (frames in which the bond is present) and `bond_of_entry` (table row of every entry:
    the sparse presence matrix frames x bonds); the counts summed over the frames."""

    def __init__(self, per_frame, frame_offsets, triples, dist_da, dist_ha, angle, table, occupancy, bond_of_entry, don_count, acc_count, cmap):
        self.per_frame, self.frame_offsets = per_frame, frame_offsets
        self.triples, self.dist_da, self.dist_ha, self.angle = triples, dist_da, dist_ha, angle
        self.table, self.occupancy, self.bond_of_entry = table, occupancy, bond_of_entry
        self.don_count, self.acc_count, self.map = don_count, acc_count, cmap
        self._engine, self._serial = None, None

    def lifetimes(self, groups=None, ngroups=None, max_lag=None, origin_stride=1, gap=0, want=LIFETIME_OUTPUTS):
        """Lifetime correlations of the block's bonds (molar_hip_hbonds_frames_lifetimes): Engine.lifetimes on the presence
        matrix the engine still holds on the device - rows are the rows of `table`, nothing is copied out and back.  Valid
        until the engine's next hydrogen-bond call, of a frame or of another block: MolarHipError NO_SEARCH after that (the
        engine numbers its blocks, and this one remembers its number)."""
        if self._engine is None:
            raise ValueError("HBondsBlock.lifetimes: the block was not made by Engine.hbonds_frames")
        return self._engine._hbonds_block_lifetimes(self._serial, self.bond_of_entry, groups, ngroups, max_lag, origin_stride, gap, want)


class Lifetimes:
    """Result of a lifetimes call: `inter` / `cont` [ngroups, max_lag + 1] - the numerators of the intermittent and the continuous
    correlation -, `run_hist` [ngroups, F + 1], `events` / `longest` / `present` [nrows] (None for what was not asked for), and
    `count` [max_lag + 1] (numpy uint64): the time origins of every lag.  `lifetime_curves` normalises."""

    def __init__(self, inter, cont, run_hist, events, longest, present, count, nframes, origin_stride):
        self.inter, self.cont, self.run_hist = inter, cont, run_hist
        self.events, self.longest, self.present = events, longest, present
        self.count, self.nframes, self.origin_stride = count, nframes, origin_stride


def lifetime_count(nframes, max_lag, origin_stride=1):
    """count[tau], tau = 0 .. max_lag: the origins t = 0, origin_stride, ... with t + tau <= nframes - 1 (numpy uint64)."""
    tau = np.arange(int(max_lag) + 1, dtype=np.int64)
    return ((int(nframes) - 1 - tau) // int(origin_stride) + 1).astype(np.uint64)


def lifetimes_plan(nframes, nrows, ngroups=1, want_cont=True):
    """(workspace_bytes, words_per_row) of a lifetimes call of these sizes (molar_hip_lifetimes_plan): the device workspace - the
    bit matrix, the origin masks and, with want_cont, one histogram per group - and the 64-bit words of a row.  A host
    function: no GPU is needed."""
    ws, wpr = C.c_size_t(0), C.c_uint32(0)
    check(_lib.load().molar_hip_lifetimes_plan(int(nframes), int(nrows), int(ngroups), 1 if want_cont else 0, C.addressof(ws), C.addressof(wpr)))
    return int(ws.value), int(wpr.value)


LifetimeCurves = collections.namedtuple("LifetimeCurves", ["tau", "c_inter", "c_cont", "tau_inter", "tau_cont"])


def lifetime_curves(res, dt=1.0):
    """The normalised correlations of a `Lifetimes` in float64 on the host: C_x(tau) = (x[tau] / count[tau]) / (x[0] / count[0])
    for x = inter, cont ([ngroups, max_lag + 1]; NaN where a denominator is 0; None for a curve that was not computed), and
    their trapezoid integrals over tau * dt, the lifetimes [ngroups].  Returns LifetimeCurves(tau, c_inter, c_cont, tau_inter,
    tau_cont) with tau = lag * dt."""
    count = np.asarray(res.count, np.float64)
    tau = np.arange(count.shape[0], dtype=np.float64) * float(dt)

    def curve(x):
        if x is None:
            return None, None
        x = np.asarray(x.cpu() if _is_torch(x) else x).astype(np.float64)
        with np.errstate(divide="ignore", invalid="ignore"):
            c = (x / count[None, :]) / (x[:, :1] / count[0])
        integral = ((c[:, 1:] + c[:, :-1]) * 0.5 * np.diff(tau)[None, :]).sum(axis=1)
        return c, integral

    (ci, ti), (cc, tc) = curve(res.inter), curve(res.cont)
    return LifetimeCurves(tau, ci, cc, ti, tc)


def _lifetimes_call(call, F, R, groups, ngroups, max_lag, origin_stride, want, like):
    """The shared end of Engine.lifetimes and HBondsBlock.lifetimes: labels, outputs of the kind of `like`, the call."""
    want = (want,) if isinstance(want, str) else tuple(want)
    unknown = set(want) - set(LIFETIME_OUTPUTS)
    if unknown:
        raise ValueError(f"lifetimes: unknown outputs {sorted(unknown)}")
    groups = _u32(groups)
    if groups is None:
        G, ga = 1, None
    else:
        if ngroups is None:
            if _is_torch(groups):
                raise ValueError("lifetimes: ngroups is needed with labels in a tensor")
            ngroups = int(groups.max()) + 1 if groups.shape[0] else 0
        G, ga = int(ngroups), _addr(groups)[0]
    L = max(F - 1, 0) if max_lag is None else int(max_lag)
    dev = _is_torch(like)
    shapes = {"inter": (G, L + 1), "cont": (G, L + 1), "run_hist": (G, F + 1), "events": (R,), "longest": (R,), "present": (R,)}
    out = {}
    for name in LIFETIME_OUTPUTS:
        wide = name in ("inter", "cont", "run_hist")
        if name not in want:
            out[name] = None
        elif dev:
            import torch
            out[name] = torch.zeros(shapes[name], dtype=torch.int64 if wide else torch.int32, device=like.device)
        else:
            out[name] = np.zeros(shapes[name], np.uint64 if wide else np.uint32)
    if dev:
        import torch
        torch.cuda.current_stream().synchronize()          # torch made the outputs on ITS stream; the engine writes on its own
    check(call(ga, G, L, [_addr(out[name])[0] for name in LIFETIME_OUTPUTS]))
    count = lifetime_count(F, L, origin_stride)
    return Lifetimes(out["inter"], out["cont"], out["run_hist"], out["events"], out["longest"], out["present"], count, F, int(origin_stride))


def hydrogens_csr(hydrogens, ndonors):
    """The donors' hydrogens as the CSR (offsets [ndonors + 1], idx) the C ABI takes (uint64 numpy, or int64 tensors when that is
    what was given), from one atom index per donor (a 1-D array of ndonors entries), a list of lists (none, one or several per
    donor), or the tuple (offsets, idx) itself."""
    if isinstance(hydrogens, tuple):
        if len(hydrogens) != 2:
            raise ValueError("hydrogens: a tuple is (offsets, idx)")
        off, idx = _u64(hydrogens[0]), _u64(hydrogens[1])
        if off.ndim != 1 or idx.ndim != 1 or off.shape[0] != ndonors + 1:
            raise ValueError(f"hydrogens: {ndonors} donors need {ndonors + 1} offsets")
        return off, idx
    if _is_torch(hydrogens) or (isinstance(hydrogens, np.ndarray) and hydrogens.dtype != object):
        idx = _u64(hydrogens)
        if idx.ndim != 1 or idx.shape[0] != ndonors:
            raise ValueError(f"hydrogens: one index per donor means {ndonors} entries")
        return np.arange(ndonors + 1, dtype=np.uint64), idx
    rows = list(hydrogens)
    if len(rows) != ndonors:
        raise ValueError(f"hydrogens: {len(rows)} entries for {ndonors} donors")
    if all(np.ndim(r) == 0 for r in rows):
        return np.arange(ndonors + 1, dtype=np.uint64), np.asarray(rows, dtype=np.uint64).reshape(ndonors)
    rows = [np.atleast_1d(np.asarray(r, dtype=np.uint64)) for r in rows]
    off = np.zeros(ndonors + 1, np.uint64)
    np.cumsum([r.shape[0] for r in rows], out=off[1:])
    return off, (np.concatenate(rows) if rows else np.zeros(0, np.uint64)).astype(np.uint64)


def _hbonds_arrays(n, like, ncols):
    """([n, 3] triples, ncols float64 columns) for a fill call: CUDA tensors when the coordinates are one."""
    if _is_torch(like):
        import torch
        return (torch.empty((n, 3), dtype=torch.int32, device=like.device),
                [torch.empty(n, dtype=torch.float64, device=like.device) for _ in range(ncols)])
    return np.empty((n, 3), np.uint32), [np.empty(n, np.float64) for _ in range(ncols)]


def _hbonds_u32(n, like):
    if _is_torch(like):
        import torch
        return torch.empty(n, dtype=torch.int32, device=like.device)
    return np.empty(n, np.uint32)


class Sasa:
    """Result of a surface-area call, with pymolar's getters: `areas` (per selected atom, nm^2), `total_area` (their
    sum in double) and, when asked for, `exposed` (points of each atom that no neighbour buries).  After a `sasa_vol`
    call also `volumes` (per selected atom, nm^3) and `total_volume`; both are None when not computed."""

    def __init__(self, areas, total_area, exposed=None, volumes=None, total_volume=None):
        self.areas, self.total_area, self.exposed = areas, total_area, exposed
        self.volumes, self.total_volume = volumes, total_volume


def sasa_points(npoints, dtype=np.float32):
    """The point table u_k[npoints, 3] of the surface-area calls (molar_hip_sasa_points / _f64); needs no GPU."""
    real = np.dtype(dtype)
    if real not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError("sasa_points: dtype must be float32 or float64")
    npoints = int(npoints) if 1 <= int(npoints) <= 0xFFFFFFFF else 0      # the library rejects it with its own message
    out = np.zeros((max(npoints, 1), 3), real)
    lib = _lib.load()
    fn = lib.molar_hip_sasa_points if real == np.float32 else lib.molar_hip_sasa_points_f64
    check(fn(npoints, out.ctypes.data))
    return out


def _sasa_call(fn, ctx, xyz, vdw, idx, probe, npoints, want_exposed, real, want_volumes=False):
    """One frame through molar_hip_sasa / _f64 or, with want_volumes, molar_hip_sasa_vol / _f64: results live where the
    coordinates live."""
    natoms = xyz.shape[0] if xyz.ndim == 2 else xyz.shape[0] // 3
    n = natoms if idx is None else idx.shape[0]
    assert vdw.shape[0] == n, "one radius per selected atom"
    if not 1 <= int(npoints) <= 0xFFFFFFFF:
        npoints = 0                                      # the library rejects it with its own message
    total = C.c_double(0.0)
    if _is_torch(xyz):
        import torch
        areas = torch.zeros(n, dtype=torch.float32 if real == np.float32 else torch.float64, device=xyz.device)
        exposed = torch.zeros(n, dtype=torch.int32, device=xyz.device) if want_exposed else None
    else:
        areas = np.zeros(n, real)
        exposed = np.zeros(n, np.uint32) if want_exposed else None
    xa, k1 = _addr(xyz); ia, k2 = _addr(idx); va, k3 = _addr(vdw); aa, k4 = _addr(areas); ea, k5 = _addr(exposed)
    if not want_volumes:
        check(fn(ctx, xa, natoms, ia, n, va, probe, int(npoints), aa if n else None, ea if n else None, C.byref(total)))
        return Sasa(areas, float(total.value), exposed)
    volumes = areas.clone() if _is_torch(xyz) else areas.copy()            # zeros of the same kind
    total_volume = C.c_double(0.0)
    oa, k6 = _addr(volumes)
    check(fn(ctx, xa, natoms, ia, n, va, probe, int(npoints), aa if n else None, ea if n else None, C.byref(total), oa if n else None,
             C.byref(total_volume)))
    return Sasa(areas, float(total.value), exposed, volumes, float(total_volume.value))


def rmsd_matrix_plan(nframes1, nframes2, n):
    """(workspace_bytes, ksplits) of an rmsd_matrix call of these sizes (molar_hip_rmsd_matrix_plan; nframes2 = 0: the
    symmetric form).  A host function: no GPU is needed."""
    ws, ks = C.c_size_t(0), C.c_uint32(0)
    check(_lib.load().molar_hip_rmsd_matrix_plan(int(nframes1), int(nframes2), int(n), C.addressof(ws), C.addressof(ks)))
    return int(ws.value), int(ks.value)


def fluct_plan(nframes, n, want_cov=True):
    """(workspace_bytes, ksplits) of a fluctuations call of these sizes (molar_hip_fluct_plan).  A host function: no GPU is
    needed."""
    ws, ks = C.c_size_t(0), C.c_uint32(0)
    check(_lib.load().molar_hip_fluct_plan(int(nframes), int(n), 1 if want_cov else 0, C.addressof(ws), C.addressof(ks)))
    return int(ws.value), int(ks.value)


def _frame_block(x, real):
    """(array, F, natoms, frame stride in elements) of frames [F, natoms, 3]; read in place when each frame is contiguous."""
    if _is_torch(x):
        import torch
        assert x.dtype == (torch.float32 if real == np.float32 else torch.float64) and x.ndim == 3 and x.shape[2] == 3
        inner = x.stride(2) == 1 and x.stride(1) == 3              # each frame contiguous (a single frame too: a transposed view is not)
        ok = inner and (x.shape[0] <= 1 or x.stride(0) >= 3 * x.shape[1])
        if not ok:
            x = x.contiguous()
        stride = x.stride(0) if x.shape[0] > 1 else 3 * x.shape[1]
        return x, x.shape[0], x.shape[1], stride
    x = np.asarray(x)
    assert x.ndim == 3 and x.shape[2] == 3
    e = np.dtype(real).itemsize
    ok = x.dtype == real and (x.shape[0] <= 1 or (x.strides[2] == e and x.strides[1] == 3 * e and x.strides[0] >= 3 * e * x.shape[1]
                                                  and x.strides[0] % e == 0))
    if not ok or (x.shape[0] <= 1 and not x.flags.c_contiguous):
        x = np.ascontiguousarray(x, dtype=real)
    stride = x.strides[0] // e if x.shape[0] > 1 else 3 * x.shape[1]
    return x, x.shape[0], x.shape[1], stride


def _rmsd_matrix_call(lib, fn, ctx, frames, idx, mass, frames2, fit, out, real):
    conv = _f32 if real == np.float32 else _f64
    fr1, F1, natoms, st1 = _frame_block(frames, real)
    dev = _is_torch(fr1)
    fr2, F2, st2 = None, 0, 0
    if frames2 is not None:
        fr2, F2, natoms2, st2 = _frame_block(frames2, real)
        assert natoms2 == natoms and _is_torch(fr2) == dev, "both blocks have the same atoms and live on the same side"
    cols = F1 if fr2 is None else F2
    idx_in, mass_in = idx, mass
    idx = _u64(idx); mass = conv(mass)
    n = natoms if idx is None else idx.shape[0]
    if mass is not None:
        assert mass.shape[0] == natoms, "one mass per atom"
    if out is None:
        if dev:
            import torch
            out = torch.zeros((F1, cols), dtype=fr1.dtype, device=fr1.device)
        else:
            out = np.zeros((F1, cols), real)
    else:
        assert _is_torch(out) == dev and out.ndim == 2 and out.shape[0] >= F1
        if dev:
            assert out.dtype == fr1.dtype and (out.shape[1] == 0 or out.stride(1) == 1)
        else:
            assert out.dtype == real and (out.shape[1] == 0 or out.strides[1] == out.itemsize)
    if dev:
        ld = out.stride(0) if out.shape[0] > 1 else out.shape[1]
        oa = out.data_ptr()
    else:
        ld = out.strides[0] // out.itemsize if out.shape[0] > 1 else out.shape[1]
        oa = out.ctypes.data
    if F1 > 0 and cols > 0 and out.shape[1] < cols:
        ld = out.shape[1]                       # too narrow: the library reports it
    a1 = fr1.data_ptr() if dev else fr1.ctypes.data
    a2 = None if fr2 is None else (fr2.data_ptr() if dev else fr2.ctypes.data)
    if fr2 is not None and not a2:
        a2 = a1                                 # an empty second block still means the rectangular form
    ia, k1 = _addr(idx); ma, k2 = _addr(mass)
    if dev:
        # torch made `out` and any contiguous copy on ITS stream; the engine reads and writes on its own
        import torch
        torch.cuda.current_stream().synchronize()
    check(fn(ctx, a1, F1, st1, a2, F2, st2, natoms, ia, n, ma, 1 if fit else 0, oa, ld))
    if dev and (fr1 is not frames or fr2 is not frames2 or idx is not idx_in or mass is not mass_in):
        # a temporary copy would go back to torch's allocator with the kernels that read it still enqueued: wait for them
        check(lib.molar_hip_synchronize(ctx))
    return out


def msd_plan(nframes, n, nparticles=None, nref=0, max_lag=None, per_frame_boxes=False, want_lags=True):
    """(workspace_bytes, particle_chunk, lag_block) of an msd call of these sizes (molar_hip_msd_plan): the device workspace and
    the particles and lags a workgroup of the lag kernel owns.  nparticles=None: every atom is a particle; max_lag=None:
    nframes - 1; want_lags=False: only `disp` is asked for.  A host function: no GPU is needed."""
    P = int(n) if nparticles is None else int(nparticles)
    L = max(int(nframes) - 1, 0) if max_lag is None else int(max_lag)
    ws, pc, lb = C.c_size_t(0), C.c_uint32(0), C.c_uint32(0)
    check(_lib.load().molar_hip_msd_plan(int(nframes), int(n), P, int(nref), L, 1 if per_frame_boxes else 0, 1 if want_lags else 0,
                                         C.addressof(ws), C.addressof(pc), C.addressof(lb)))
    return int(ws.value), int(pc.value), int(lb.value)


def msd_alpha2(msd, m4, ndims):
    """The non-Gaussian parameter alpha_2 = ndims / (ndims + 2) * m4 / msd^2 - 1 per lag, in float64 (0 for a Gaussian
    displacement distribution in ndims dimensions; NaN where msd is 0, as at lag 0)."""
    msd = np.asarray(msd, np.float64)
    m4 = np.asarray(m4, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return ndims / (ndims + 2.0) * m4 / (msd * msd) - 1.0


def msd_diffusion(msd, dt, lo, hi, ndims):
    """(slope, intercept, D) of the least-squares line through (tau * dt, msd[tau]) for the lags lo .. hi inclusive;
    D = slope / (2 ndims) (the Einstein relation).  float64 on the host."""
    lo, hi = int(lo), int(hi)
    y = np.asarray(msd, np.float64)[lo:hi + 1]
    assert y.shape[0] >= 2, "a line needs two lags"
    x = np.arange(lo, hi + 1, dtype=np.float64) * float(dt)
    xm, ym = x.mean(), y.mean()
    slope = float(((x - xm) * (y - ym)).sum() / ((x - xm) ** 2).sum())
    return slope, float(ym - slope * xm), slope / (2.0 * ndims)


Msd = collections.namedtuple("Msd", ["msd", "m4", "msd_particle", "disp"])


def _msd_call(lib, fn, ctx, frames, idx, mass, boxes, pbc, groups, ref_idx, max_lag, origin_stride, dims, want_msd, want_m4, per_particle,
              want_disp, out, real):
    conv = _f32 if real == np.float32 else _f64
    fr, F, natoms, stride = _frame_block(frames, real)
    dev = _is_torch(fr)
    given_in = (idx, mass, boxes, groups, ref_idx)
    idx = _u64(idx); mass = conv(mass); groups = _u64(groups); ref_idx = _u64(ref_idx)
    box_stride = 0
    if boxes is None:
        pbc = 0                                  # already unwrapped: no image is removed
    else:
        boxes = conv(boxes)
        if boxes.ndim == 2 and tuple(boxes.shape) == (3, 3):
            boxes = (boxes.T.contiguous() if _is_torch(boxes) else np.ascontiguousarray(boxes.T)).reshape(9)      # rows -> column-major
        if boxes.ndim == 2:
            assert tuple(boxes.shape) == (F, 9), "per-frame boxes are [F, 9], column-major"
            box_stride = 9
        else:
            assert tuple(boxes.shape) == (9,), "a box is [9] column-major or [3, 3]"
    n = natoms if idx is None else idx.shape[0]
    P = n if groups is None else groups.shape[0] - 1
    nref = 0 if ref_idx is None else ref_idx.shape[0]
    if mass is not None:
        assert mass.shape[0] == natoms, "one mass per atom"
    L = max(F - 1, 0) if max_lag is None else int(max_lag)
    want = (bool(want_msd), bool(want_m4), bool(per_particle), bool(want_disp))
    shapes = ((L + 1,), (L + 1,), (P, L + 1), (F, P, 3))
    given = tuple(out) if out is not None else (None,) * 4
    res = []
    for w, shape, g in zip(want, shapes, given):
        if not w:
            res.append(None)
        elif g is not None:
            assert _is_torch(g) == dev and tuple(g.shape) == shape
            assert (g.dtype == fr.dtype and g.is_contiguous()) if dev else (g.dtype == real and g.flags.c_contiguous)
            res.append(g)
        elif dev:
            import torch
            res.append(torch.zeros(shape, dtype=fr.dtype, device=fr.device))
        else:
            res.append(np.zeros(shape, real))
    addr = [None if r is None else (r.data_ptr() if dev else r.ctypes.data) for r in res]
    fa = fr.data_ptr() if dev else fr.ctypes.data
    ia, k1 = _addr(idx); ma, k2 = _addr(mass); ba, k3 = _addr(boxes); ga, k4 = _addr(groups); ra, k5 = _addr(ref_idx)
    if dev:
        # torch made the outputs and any contiguous copy on ITS stream; the engine reads and writes on its own
        import torch
        torch.cuda.current_stream().synchronize()
    check(fn(ctx, fa, F, stride, natoms, ia, n, ma, ba, box_stride, int(pbc), ga, P, ra, nref, L, int(origin_stride), int(dims),
             addr[0], addr[1], addr[2], L + 1, addr[3]))
    if dev and (fr is not frames or any(a is not b for a, b in zip((idx, mass, boxes, groups, ref_idx), given_in))):
        # a temporary copy would go back to torch's allocator with the kernels that read it still enqueued: wait for them
        check(lib.molar_hip_synchronize(ctx))
    return Msd(*res)


Density = collections.namedtuple("Density", ["density", "count", "outside", "centre", "binvol", "weight_scale_log2", "grid"])
DensityGrid = collections.namedtuple("DensityGrid", ["mode", "nbins", "lo", "hi", "centre_dims"])
DENSITY_BOX, DENSITY_LAB = 0, 1


def profile_grid(axis, nbins, centre=False):
    """The grid of a profile along box vector `axis` (0, 1, 2) in fractional coordinates (gmx density -relative): `nbins` bins
    along it, the other two dimensions integrated over.  centre=True: the profile is centred per frame on the centre set of
    the call (the circular mean on a periodic dimension), which then sits at the middle of the range."""
    axis = int(axis)
    assert axis in (0, 1, 2)
    nb = [1, 1, 1]
    nb[axis] = int(nbins)
    return DensityGrid(DENSITY_BOX, tuple(nb), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), (1 << axis) if centre else 0)


def map_grid(nbins_xy, centre=False):
    """The grid of a lateral map in fractional coordinates (gmx densmap): nbins_xy = (nx, ny), z integrated over."""
    nx, ny = (int(v) for v in nbins_xy)
    return DensityGrid(DENSITY_BOX, (nx, ny, 1), (0.0, 0.0, 0.0), (1.0, 1.0, 1.0), 3 if centre else 0)


def volume_grid(lo, hi, nbins, centre=False):
    """The grid of a volume map in the coordinates of the frames as they are (VMD volmap, gmx spatial on fitted frames): the
    half-open range lo .. hi with nbins = (nx, ny, nz) bins.  centre=True: lo and hi are relative to the centre of the
    call's centre set in each frame."""
    lo = tuple(float(v) for v in lo)
    hi = tuple(float(v) for v in hi)
    nb = tuple(int(v) for v in nbins)
    assert len(lo) == len(hi) == len(nb) == 3
    return DensityGrid(DENSITY_LAB, nb, lo, hi, 7 if centre else 0)


def _grid_struct(grid):
    g = _lib.DensityGrid()
    g.mode = int(grid.mode)
    for d in range(3):
        g.nbins[d] = int(grid.nbins[d])
        g.lo[d] = float(grid.lo[d])
        g.hi[d] = float(grid.hi[d])
    g.centre_dims = int(grid.centre_dims)
    return g


def density_plan(nframes, n, grid, ngroups=1):
    """(workspace_bytes, frame_chunk, atom_chunk, lds_cells) of a density call of these sizes (molar_hip_density_plan): the
    device workspace, the frames whose integer bins are held at once, the atoms of one frame a workgroup bins, and the
    largest ngroups * bins the on-chip binning kernel takes.  A host function: no GPU is needed."""
    g = _grid_struct(grid)
    ws, fc, ac, lc = C.c_size_t(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    check(_lib.load().molar_hip_density_plan(int(nframes), int(n), int(ngroups), C.addressof(g), C.addressof(ws), C.addressof(fc),
                                             C.addressof(ac), C.addressof(lc)))
    return int(ws.value), int(fc.value), int(ac.value), int(lc.value)


def density_axis(grid, d, box=None):
    """The centres of the bins along dimension d, float64.  LAB grid: lo + (i + 1/2) (hi - lo) / nbins (relative to the centre
    when the grid is centred).  BOX grid: the fractional (i + 1/2) / nbins, minus 1/2 when dimension d is centred (the centre
    set then sits at 0); with `box` ([9] column-major or [3, 3] rows: one box, the mean box of the block say) times the
    length of box vector d."""
    nb = int(grid.nbins[d])
    u = (np.arange(nb, dtype=np.float64) + 0.5) / nb
    if grid.mode == DENSITY_LAB:
        return grid.lo[d] + u * (grid.hi[d] - grid.lo[d])
    if grid.centre_dims >> d & 1:
        u = u - 0.5
    if box is None:
        return u
    b = np.asarray(box, np.float64)
    vec = b[d] if b.ndim == 2 else b.reshape(9)[3 * d:3 * d + 3]
    return u * float(np.sqrt((vec * vec).sum()))


def density_symmetrize(density, grid, d):
    """The mean of a density and its mirror image about the middle of the range of dimension d (gmx density -symm), for an
    array whose last three dimensions are the grid's (or one flattened over them); float64 on the host."""
    a = np.asarray(density, np.float64)
    shape = a.shape
    nb = tuple(int(v) for v in grid.nbins)
    if shape[-3:] != nb:
        a = a.reshape(shape[:-1] + nb)
    out = 0.5 * (a + np.flip(a, axis=a.ndim - 3 + d))
    return out.reshape(shape)


def _density_call(lib, fn, ctx, frames, grid, idx, weight, labels, ngroups, boxes, pbc, centre_idx, centre_weight, want, out, real):
    conv = _f32 if real == np.float32 else _f64
    fr, F, natoms, stride = _frame_block(frames, real)
    dev = _is_torch(fr)
    given_in = (idx, weight, labels, boxes, centre_idx, centre_weight)
    idx = _u64(idx); weight = conv(weight); labels = _u32(labels); centre_idx = _u64(centre_idx); centre_weight = conv(centre_weight)
    box_stride = 0
    if boxes is not None:
        boxes = conv(boxes)
        if boxes.ndim == 2 and tuple(boxes.shape) == (3, 3):
            boxes = (boxes.T.contiguous() if _is_torch(boxes) else np.ascontiguousarray(boxes.T)).reshape(9)      # rows -> column-major
        if boxes.ndim == 2:
            assert tuple(boxes.shape) == (F, 9), "per-frame boxes are [F, 9], column-major"
            box_stride = 9
        else:
            assert tuple(boxes.shape) == (9,), "a box is [9] column-major or [3, 3]"
    n = natoms if idx is None else idx.shape[0]
    ncentre = 0 if centre_idx is None else centre_idx.shape[0]
    G = 1
    if labels is not None:
        assert labels.shape[0] == n, "one label per selected atom"
        G = int(ngroups) if ngroups is not None else (int(labels.max()) + 1 if n else 1)
    for w in (weight, centre_weight):
        if w is not None:
            assert w.shape[0] == natoms, "one weight per atom"
    nbins = tuple(int(v) for v in grid.nbins)
    names = ("density", "count", "outside", "centre", "binvol")
    want = names if want is None else tuple(want)
    shapes = ((G,) + nbins, (G,) + nbins, (F,), (F, 3), (F,))
    given = tuple(out[:5]) if out is not None else (None,) * 5
    res = []
    for name, shape, g in zip(names, shapes, given):
        integer = name in ("count", "outside")
        if name not in want:
            res.append(None)
        elif g is not None:
            assert _is_torch(g) == dev and tuple(g.shape) == shape
            if dev:
                import torch
                assert g.dtype == (torch.int64 if integer else fr.dtype) and g.is_contiguous()
            else:
                assert g.dtype == (np.uint64 if integer else real) and g.flags.c_contiguous
            res.append(g)
        elif dev:
            import torch
            res.append(torch.zeros(shape, dtype=torch.int64 if integer else fr.dtype, device=fr.device))
        else:
            res.append(np.zeros(shape, np.uint64 if integer else real))
    addr = [None if r is None else (r.data_ptr() if dev else r.ctypes.data) for r in res]
    gs = _grid_struct(grid)
    scale = C.c_int32(0)
    fa = fr.data_ptr() if dev else fr.ctypes.data
    ia, k1 = _addr(idx); wa, k2 = _addr(weight); la, k3 = _addr(labels); ba, k4 = _addr(boxes); ca, k5 = _addr(centre_idx)
    cwa, k6 = _addr(centre_weight)
    if dev:
        # torch made the outputs and any contiguous copy on ITS stream; the engine reads and writes on its own
        import torch
        torch.cuda.current_stream().synchronize()
    check(fn(ctx, fa, F, stride, natoms, ia, n, wa, la, G, ba, box_stride, int(pbc), C.addressof(gs), ca, ncentre, cwa,
             addr[0], addr[1], addr[2], addr[3], addr[4], C.addressof(scale)))
    if dev and (fr is not frames or any(a is not b for a, b in zip((idx, weight, labels, boxes, centre_idx, centre_weight), given_in))):
        # a temporary copy would go back to torch's allocator with the kernels that read it still enqueued: wait for them
        check(lib.molar_hip_synchronize(ctx))
    return Density(*res, int(scale.value), grid)


InternalCoords = collections.namedtuple("InternalCoords", ["values", "hist", "map", "mean", "spread", "valid", "edges"])
IC_DISTANCE, IC_ANGLE, IC_DIHEDRAL = 2, 3, 4


def _intcoord_spec(kind, nbins, range, map_bins):
    sp = _lib.IntcoordSpec()
    sp.kind = int(kind)
    sp.nbins = int(nbins)
    sp.map_bins = int(map_bins)
    sp.reserved = 0
    if range is None:
        assert int(kind) != IC_DISTANCE or (int(nbins) == 0 and int(map_bins) == 0), "a distance histogram needs range=(lo, hi)"
        range = (0.0, 1.0)
    sp.lo, sp.hi = float(range[0]), float(range[1])
    return sp


def intcoord_plan(nframes, ntuples, kind, ngroups=1, npairs=0, npair_groups=1, nbins=0, range=None, map_bins=0, want_stats=True):
    """(workspace_bytes, frame_chunk, tuple_chunk, lds_cells) of an internal_coords call of these sizes
    (molar_hip_intcoord_plan): the device workspace (the chunk partials of mean / spread / valid), the frames and the tuples
    (or pairs) a workgroup takes, and the largest ngroups * nbins (npair_groups * map_bins^2) the on-chip histogram takes.  A
    host function: no GPU is needed."""
    sp = _intcoord_spec(kind, nbins, range, map_bins)
    ws, fc, tc, lc = C.c_size_t(0), C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
    check(_lib.load().molar_hip_intcoord_plan(int(nframes), int(ntuples), int(ngroups), int(npairs), int(npair_groups), C.addressof(sp),
                                              1 if want_stats else 0, C.addressof(ws), C.addressof(fc), C.addressof(tc), C.addressof(lc)))
    return int(ws.value), int(fc.value), int(tc.value), int(lc.value)


def intcoord_edges(kind, nbins, range=None):
    """The nbins + 1 bin edges of an internal_coords histogram (or of one side of its map), float64: lo .. hi for distances,
    0 .. pi for angles, -pi .. pi for dihedrals."""
    if int(kind) == IC_DISTANCE:
        lo, hi = (float(v) for v in range)
    elif int(kind) == IC_ANGLE:
        lo, hi = 0.0, np.pi
    else:
        lo, hi = -np.pi, np.pi
    return lo + (hi - lo) * (np.arange(int(nbins) + 1, dtype=np.float64) / int(nbins))


def intcoord_degrees(x):
    """Radians to degrees for angles, dihedrals, their means and bin edges (numpy or torch; distances and the circular
    variance are not angles)."""
    return x * (180.0 / np.pi)


def circular_std(spread):
    """The circular standard deviation sqrt(-2 ln(1 - V)) in radians of the circular variance V that internal_coords
    returns as the `spread` of dihedrals (V = 1: infinite)."""
    v = np.asarray(spread, np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.sqrt(-2.0 * np.log1p(-v))


def backbone_dihedrals(names, resids, chains=None):
    """The backbone dihedrals of a protein from per-atom columns (gro.GroTopology's names and resids; chains: an optional
    per-atom chain column).  Returns (phi, psi, omega, phi_res, psi_res, omega_res, pairs): the uint64 [n, 4] tuples
    phi = C(i-1) N CA C, psi = N CA C N(i+1), omega = CA C N(i+1) CA(i+1); for each, the index of its residue i among the
    residues in order of first appearance; and pairs [m, 2]: (row of phi, row of psi) of every residue that has both, rows
    of psi counted from len(phi) - the pairs of internal_coords(tuples=concatenate([phi, psi]), pairs=pairs).  Neighbours are
    consecutive residues of one chain whose resids differ by one; a residue that lacks a neighbour or an atom gets no tuple."""
    names = [str(n).strip() for n in names]
    resids = np.asarray(resids).astype(np.int64)
    n = len(names)
    assert resids.shape == (n,)
    chains = None if chains is None else list(chains)
    res = []                                  # (resid, chain, {name: atom})
    for a in range(n):
        key = (int(resids[a]), None if chains is None else chains[a])
        if not res or (res[-1][0], res[-1][1]) != key:
            res.append((key[0], key[1], {}))
        res[-1][2].setdefault(names[a], a)

    def linked(i, j):
        return 0 <= i and j < len(res) and res[i][1] == res[j][1] and res[j][0] == res[i][0] + 1

    def tup(*atoms):
        return None if any(a is None for a in atoms) else atoms

    phi, psi, omega, rphi, rpsi, romega, pairs = [], [], [], [], [], [], []
    for i, (_, _, at) in enumerate(res):
        t_phi = tup(res[i - 1][2].get("C"), at.get("N"), at.get("CA"), at.get("C")) if linked(i - 1, i) else None
        nxt = res[i + 1][2] if linked(i, i + 1) else None
        t_psi = tup(at.get("N"), at.get("CA"), at.get("C"), nxt.get("N")) if nxt is not None else None
        t_om = tup(at.get("CA"), at.get("C"), nxt.get("N"), nxt.get("CA")) if nxt is not None else None
        if t_phi is not None and t_psi is not None:
            pairs.append((len(phi), len(psi)))
        if t_phi is not None:
            phi.append(t_phi); rphi.append(i)
        if t_psi is not None:
            psi.append(t_psi); rpsi.append(i)
        if t_om is not None:
            omega.append(t_om); romega.append(i)
    t4 = lambda v: np.asarray(v, np.uint64).reshape(-1, 4)
    pr = np.asarray(pairs, np.uint64).reshape(-1, 2)
    pr[:, 1] += len(phi)
    return (t4(phi), t4(psi), t4(omega), np.asarray(rphi, np.int64), np.asarray(rpsi, np.int64), np.asarray(romega, np.int64), pr)


def _intcoord_call(lib, fn, ctx, frames, tuples, kind, labels, ngroups, boxes, pbc, nbins, range, pairs, pair_labels, npair_groups, map_bins, want,
                   out, real):
    conv = _f32 if real == np.float32 else _f64
    fr, F, natoms, stride = _frame_block(frames, real)
    dev = _is_torch(fr)
    given_in = (tuples, labels, boxes, pairs, pair_labels)
    tuples = _u64(tuples); labels = _u32(labels); pairs = _u64(pairs); pair_labels = _u32(pair_labels)
    assert tuples.ndim == 2 and tuples.shape[1] in (2, 3, 4), "tuples are [T, 2], [T, 3] or [T, 4]"
    kind = int(tuples.shape[1]) if kind is None else int(kind)
    assert kind == tuples.shape[1], "kind is the number of atoms per tuple"
    T = int(tuples.shape[0])
    box_stride = 0
    if boxes is not None:
        boxes = conv(boxes)
        if boxes.ndim == 2 and tuple(boxes.shape) == (3, 3):
            boxes = (boxes.T.contiguous() if _is_torch(boxes) else np.ascontiguousarray(boxes.T)).reshape(9)      # rows -> column-major
        if boxes.ndim == 2:
            assert tuple(boxes.shape) == (F, 9), "per-frame boxes are [F, 9], column-major"
            box_stride = 9
        else:
            assert tuple(boxes.shape) == (9,), "a box is [9] column-major or [3, 3]"
    else:
        pbc = 0
    G = 1
    if labels is not None:
        assert labels.shape[0] == T, "one label per tuple"
        G = int(ngroups) if ngroups is not None else (int(labels.max()) + 1 if T else 1)
    P, G2 = 0, 1
    if pairs is not None:
        assert pairs.ndim == 2 and pairs.shape[1] == 2, "pairs are [P, 2]"
        P = int(pairs.shape[0])
    if pair_labels is not None:
        assert pairs is not None and pair_labels.shape[0] == P, "one label per pair"
        G2 = int(npair_groups) if npair_groups is not None else (int(pair_labels.max()) + 1 if P else 1)
    nbins, map_bins = int(nbins), int(map_bins)
    names = ("values", "hist", "map", "mean", "spread", "valid")
    if want is None:
        want = tuple(nm for nm in names if not (nm == "hist" and nbins == 0) and not (nm == "map" and (map_bins == 0 or pairs is None)))
    want = tuple(want)
    shapes = ((F, T), (G, nbins), (G2, map_bins, map_bins), (T,), (T,), (T,))
    given = tuple(out[:6]) if out is not None else (None,) * 6
    res, ld = [], T
    for name, shape, g in zip(names, shapes, given):
        integer = name in ("hist", "map", "valid")
        if name not in want:
            res.append(None)
        elif g is not None:
            assert _is_torch(g) == dev and tuple(g.shape) == shape
            if dev:
                import torch
                assert g.dtype == (torch.int64 if integer else fr.dtype)
                if name == "values" and F > 1:
                    assert g.stride(1) == 1 and g.stride(0) >= T, "values: rows contiguous"
                    ld = int(g.stride(0))
                else:
                    assert g.is_contiguous()
            else:
                assert g.dtype == (np.uint64 if integer else real)
                if name == "values" and F > 1 and T > 0:
                    e = g.dtype.itemsize
                    assert g.strides[1] == e and g.strides[0] % e == 0 and g.strides[0] >= T * e, "values: rows contiguous"
                    ld = g.strides[0] // e
                else:
                    assert g.flags.c_contiguous
            res.append(g)
        elif dev:
            import torch
            res.append(torch.zeros(shape, dtype=torch.int64 if integer else fr.dtype, device=fr.device))
        else:
            res.append(np.zeros(shape, np.uint64 if integer else real))
    addr = [None if r is None else (r.data_ptr() if dev else r.ctypes.data) for r in res]
    sp = _intcoord_spec(kind, nbins, range, map_bins)
    fa = fr.data_ptr() if dev else fr.ctypes.data
    ta, k1 = _addr(tuples); la, k2 = _addr(labels); ba, k3 = _addr(boxes); pa, k4 = _addr(pairs); pla, k5 = _addr(pair_labels)
    if dev:
        # torch made the outputs and any contiguous copy on ITS stream; the engine reads and writes on its own
        import torch
        torch.cuda.current_stream().synchronize()
    check(fn(ctx, fa, F, stride, natoms, ta, T, la, G, ba, box_stride, int(pbc), C.addressof(sp), pa, P, pla, G2,
             addr[0], ld, addr[1], addr[2], addr[3], addr[4], addr[5]))
    if dev and (fr is not frames or any(a is not b for a, b in zip((tuples, labels, boxes, pairs, pair_labels), given_in))):
        # a temporary copy would go back to torch's allocator with the kernels that read it still enqueued: wait for them
        check(lib.molar_hip_synchronize(ctx))
    edges = None
    if nbins or map_bins:
        edges = intcoord_edges(kind, nbins if nbins else map_bins, range)
    return InternalCoords(*res, edges)


VectorCorrelations = collections.namedtuple("VectorCorrelations", ["c1", "c2", "c1_vec", "c2_vec", "nvalid", "mean", "s2", "bad_frames", "lags"])
TCF_UNIT, TCF_RAW = 0, 1


def _tcf_spec(kind, mode, dims):
    sp = _lib.TcfSpec()
    sp.kind = int(kind)
    sp.mode = {"unit": TCF_UNIT, "raw": TCF_RAW}.get(mode, mode)
    sp.dims = int(dims)
    sp.reserved = 0
    return sp


def tcf_plan(nframes, nvectors, ngroups=1, max_lag=None, per_frame_boxes=False, want_lags=True, want_groups=True):
    """(workspace_bytes, frame_chunk, vec_chunk, lag_block, lags_per_lane, segment, window) of a vector_correlations call of
    these sizes (molar_hip_tcf_plan): the device workspace and the launch shape - the frames a lane of the vector stage walks,
    the vectors and the lags a workgroup of the lag kernel owns, the lags of one lane, the origins staged at a time and the
    frames they reach.  max_lag=None: nframes - 1; want_lags=False: only mean / s2 / bad_frames / nvalid are asked for;
    want_groups=False: no group curve (c1, c2).  A host function: no GPU is needed."""
    L = max(int(nframes) - 1, 0) if max_lag is None else int(max_lag)
    ws = C.c_size_t(0)
    u = [C.c_uint32(0) for _ in range(6)]
    check(_lib.load().molar_hip_tcf_plan(int(nframes), int(nvectors), int(ngroups), L, 1 if per_frame_boxes else 0, 1 if want_lags else 0,
                                         1 if want_groups else 0, C.addressof(ws), *(C.addressof(x) for x in u)))
    return (int(ws.value),) + tuple(int(x.value) for x in u)


def tcf_lags(nframes, max_lag=None, origin_stride=1):
    """n(tau) = (F - 1 - tau) // origin_stride + 1 for tau = 0 .. max_lag (None: F - 1), int64: the time origins that enter
    every lag of a vector_correlations (or msd) call."""
    F = int(nframes)
    L = F - 1 if max_lag is None else int(max_lag)
    assert 0 <= L < F and int(origin_stride) >= 1
    return (F - 1 - np.arange(L + 1, dtype=np.int64)) // min(int(origin_stride), F) + 1


def correlation_time(curve, dt):
    """The integral of a correlation curve over tau * dt by the trapezoid rule, from lag 0 up to its first zero crossing (the
    crossing itself interpolated linearly) or, without one, to its end; float64.  A curve that starts at or below 0: 0."""
    y = np.asarray(curve, np.float64)
    assert y.ndim == 1 and y.shape[0] >= 1
    below = np.nonzero(y <= 0.0)[0]
    if below.size == 0:
        return float(dt) * float(((y[1:] + y[:-1]) * 0.5).sum())
    k = int(below[0])
    if k == 0:
        return 0.0
    whole = float(((y[1:k] + y[:k - 1]) * 0.5).sum())
    frac = y[k - 1] / (y[k - 1] - y[k])                  # where the line from lag k - 1 to lag k meets zero
    return float(dt) * (whole + 0.5 * float(y[k - 1]) * float(frac))


def angle_vectors(values):
    """An angle series [F, T] (the `values` of internal_coords for dihedrals, radians; numpy or torch) as the block
    [F, T, 3] of (cos, sin, 0): vector_correlations(block, arange(T), mode="raw") then gives <cos(phi(t + tau) - phi(t))>, the
    dihedral autocorrelation.  A NaN angle gives a bad frame of its vector."""
    if _is_torch(values):
        import torch
        return torch.stack([torch.cos(values), torch.sin(values), torch.zeros_like(values)], dim=-1).contiguous()
    v = np.asarray(values)
    return np.ascontiguousarray(np.stack([np.cos(v), np.sin(v), np.zeros_like(v)], axis=-1))


def _tcf_call(lib, fn, ctx, frames, tuples, kind, labels, ngroups, boxes, pbc, mode, dims, max_lag, origin_stride, want, out, real):
    conv = _f32 if real == np.float32 else _f64
    fr, F, natoms, stride = _frame_block(frames, real)
    dev = _is_torch(fr)
    given_in = (tuples, labels, boxes)
    tuples = _u64(tuples); labels = _u32(labels)
    if tuples.ndim == 1:
        tuples = tuples.reshape(-1, 1)
    assert tuples.ndim == 2 and tuples.shape[1] in (1, 2, 3), "tuples are [V], [V, 1], [V, 2] or [V, 3]"
    kind = int(tuples.shape[1]) if kind is None else int(kind)
    assert kind == tuples.shape[1], "kind is the number of atoms per tuple"
    V = int(tuples.shape[0])
    box_stride = 0
    if boxes is not None and kind >= 2:
        boxes = conv(boxes)
        if boxes.ndim == 2 and tuple(boxes.shape) == (3, 3):
            boxes = (boxes.T.contiguous() if _is_torch(boxes) else np.ascontiguousarray(boxes.T)).reshape(9)      # rows -> column-major
        if boxes.ndim == 2:
            assert tuple(boxes.shape) == (F, 9), "per-frame boxes are [F, 9], column-major"
            box_stride = 9
        else:
            assert tuple(boxes.shape) == (9,), "a box is [9] column-major or [3, 3]"
    else:
        boxes, pbc = None, 0
    G = 1
    if labels is not None:
        assert labels.shape[0] == V, "one label per vector"
        G = int(ngroups) if ngroups is not None else (int(labels.max()) + 1 if V else 1)
    L = max(F - 1, 0) if max_lag is None else int(max_lag)
    sp = _tcf_spec(kind, mode, dims)
    names = ("c1", "c2", "c1_vec", "c2_vec", "nvalid", "mean", "s2", "bad_frames")
    if want is None:
        want = tuple(nm for nm in ("c1", "c2", "nvalid", "mean", "s2", "bad_frames") if sp.mode == TCF_UNIT or nm not in ("c2", "s2"))
    want = tuple(want)
    assert all(nm in names for nm in want), "want holds names of VectorCorrelations"
    shapes = ((G, L + 1), (G, L + 1), (V, L + 1), (V, L + 1), (G,), (V, 3), (V,), (V,))
    given = tuple(out[:8]) if out is not None else (None,) * 8
    res, ld = [], L + 1
    for name, shape, g in zip(names, shapes, given):
        if name not in want:
            res.append(None)
            continue
        if dev:
            import torch
            dt = torch.int64 if name == "nvalid" else torch.int32 if name == "bad_frames" else fr.dtype
        else:
            dt = np.uint64 if name == "nvalid" else np.uint32 if name == "bad_frames" else real
        if g is not None:
            assert _is_torch(g) == dev and tuple(g.shape) == shape and g.dtype == dt
            if name in ("c1_vec", "c2_vec") and V > 1:
                if dev:
                    assert g.stride(1) == 1 and g.stride(0) >= L + 1, f"{name}: rows contiguous"
                    row = int(g.stride(0))
                else:
                    e = g.dtype.itemsize
                    assert g.strides[1] == e and g.strides[0] % e == 0 and g.strides[0] >= (L + 1) * e, f"{name}: rows contiguous"
                    row = g.strides[0] // e
                assert ld in (L + 1, row) or row == L + 1, "c1_vec and c2_vec share one row stride"
                ld = max(ld, row)
            else:
                assert g.is_contiguous() if dev else g.flags.c_contiguous
            res.append(g)
        elif dev:
            res.append(torch.zeros(shape, dtype=dt, device=fr.device))
        else:
            res.append(np.zeros(shape, dt))
    if ld != L + 1:
        for name, r in zip(names, res):
            if name in ("c1_vec", "c2_vec") and r is not None and V > 1:
                row = int(r.stride(0)) if dev else r.strides[0] // r.dtype.itemsize
                assert row == ld, "c1_vec and c2_vec share one row stride"
    addr = [None if r is None else (r.data_ptr() if dev else r.ctypes.data) for r in res]
    fa = fr.data_ptr() if dev else fr.ctypes.data
    ta, k1 = _addr(tuples); la, k2 = _addr(labels); ba, k3 = _addr(boxes)
    if dev:
        # torch made the outputs and any contiguous copy on ITS stream; the engine reads and writes on its own
        import torch
        torch.cuda.current_stream().synchronize()
    check(fn(ctx, fa, F, stride, natoms, ta, V, la, G, ba, box_stride, int(pbc), C.addressof(sp), L, int(origin_stride),
             addr[0], addr[1], addr[2], addr[3], ld, addr[4], addr[5], addr[6], addr[7]))
    if dev and (fr is not frames or any(a is not b for a, b in zip((tuples, labels, boxes), given_in))):
        # a temporary copy would go back to torch's allocator with the kernels that read it still enqueued: wait for them
        check(lib.molar_hip_synchronize(ctx))
    lags = tcf_lags(F, L, origin_stride) if F > 0 and int(origin_stride) >= 1 and L < F else None
    return VectorCorrelations(*res, lags)


StructureFactor = collections.namedtuple("StructureFactor", ["rho", "frame_ok", "rho_mean", "sab", "shell", "shell_count", "grid"])
SfactorGrid = collections.namedtuple("SfactorGrid", ["hmax", "qmin", "dq", "nshells"])


def sfactor_grid(hmax, qmin=0.0, dq=0.0, nshells=0):
    """The reciprocal lattice of a structure_factor call: Miller indices h in [0, H], k in [-K, K], l in [-L, L] with
    hmax = (H, K, L) - (H, K, 0) is a lateral analysis, (H, 0, 0) the Fourier series of a profile - and `nshells` shells
    of |q| of width `dq` from `qmin` (0: no shells)."""
    hm = tuple(int(v) for v in hmax)
    assert len(hm) == 3 and all(v >= 0 for v in hm)
    return SfactorGrid(hm, float(qmin), float(dq), int(nshells))


def _sfactor_struct(grid):
    g = _lib.SfactorGrid()
    for d in range(3):
        g.hmax[d] = int(grid.hmax[d])
    g.qmin = float(grid.qmin)
    g.dq = float(grid.dq)
    g.nshells = int(grid.nshells)
    g.reserved = 0
    return g


def sfactor_plan(nframes, n, grid, ngroups=1):
    """(workspace_bytes, layout, row_block, col_block, atom_chunk, ksplits, frame_block) of a structure_factor call of these
    sizes (molar_hip_sfactor_plan): the device workspace; the layout (0: rows enumerate (h, k) and columns l; 1, for L = 0 with
    K > 0: rows k and columns h); the block of rows and columns of a workgroup; the atoms of a K split and how many splits n
    atoms make; the frames whose rho is held at once.  The environment variables MOLAR_HIP_SFACTOR_ATOM_CHUNK and
    MOLAR_HIP_SFACTOR_FRAME_BLOCK override the last two, here and in the call.  A host function: no GPU is needed."""
    g = _sfactor_struct(grid)
    ws = C.c_size_t(0)
    u = [C.c_uint32(0) for _ in range(6)]
    check(_lib.load().molar_hip_sfactor_plan(int(nframes), int(n), int(ngroups), C.addressof(g), C.addressof(ws), *(C.addressof(x) for x in u)))
    return (int(ws.value),) + tuple(int(x.value) for x in u)


def sfactor_miller(hmax):
    """(m [Q, 3] int64, canonical [Q] bool): the Miller indices (h, k, l) of every lattice index of a grid with this hmax, index
    (h (2K + 1) + (k + K)) (2L + 1) + (l + L), and the mask of the canonical half-space the shells are averaged over (h > 0,
    or h = 0 and k > 0, or h = k = 0 and l > 0: one of every pair m, -m, never m = 0)."""
    H, K, L = (int(v) for v in hmax)
    h, k, l = np.meshgrid(np.arange(H + 1, dtype=np.int64), np.arange(-K, K + 1, dtype=np.int64), np.arange(-L, L + 1, dtype=np.int64), indexing="ij")
    m = np.stack([h.ravel(), k.ravel(), l.ravel()], axis=1)
    canonical = (m[:, 0] > 0) | ((m[:, 0] == 0) & (m[:, 1] > 0)) | ((m[:, 0] == 0) & (m[:, 1] == 0) & (m[:, 2] > 0))
    return m, canonical


def _boxes_colmajor(boxes):
    """[9] or [F, 9] column-major float64 from [9], [3, 3] rows or [F, 9]."""
    b = np.asarray(boxes, np.float64)
    if b.ndim == 2 and b.shape == (3, 3):
        b = np.ascontiguousarray(b.T).reshape(9)
    assert b.shape[-1] == 9 and b.ndim in (1, 2), "a box is [9] column-major or [3, 3], per-frame boxes are [F, 9]"
    return b


def sfactor_qvectors(boxes, hmax):
    """q(m) = 2 pi inv(box)^T m of every lattice index, float64: [Q, 3] for one box ([9] column-major or [3, 3] rows),
    [F, Q, 3] for per-frame boxes [F, 9]."""
    b = _boxes_colmajor(boxes)
    m, _ = sfactor_miller(hmax)
    mats = b.reshape(-1, 3, 3).transpose(0, 2, 1)            # [F, row, column]
    inv = np.linalg.inv(mats)
    q = 2.0 * np.pi * np.einsum("fcr,qc->fqr", inv, m.astype(np.float64))
    return q[0] if b.ndim == 1 else q


def sfactor_shell_centres(grid):
    """The middle of every shell of |q|: qmin + (b + 1/2) dq, float64."""
    return float(grid.qmin) + (np.arange(int(grid.nshells), dtype=np.float64) + 0.5) * float(grid.dq)


def sfactor_pairs(ngroups):
    """The pairs (a, b), a <= b, in the order of sab and shell (a-major), [P, 2] int64."""
    G = int(ngroups)
    return np.array([(a, b) for a in range(G) for b in range(a, G)], np.int64).reshape(-1, 2)


def sfactor_normalize(sab, weights=None, labels=None, ngroups=None, how="n", n=None):
    """sab or shell [P, ...] of a structure_factor call divided, pair (a, b) by pair, by sqrt(N_a N_b) (how="n": the atoms of the
    two groups - the Ashcroft-Langreth partials, S_aa -> 1 at large q for unit weights) or by sqrt(W_a W_b), W_g the sum of
    w^2 over group g (how="w2").  `weights`: one per SELECTED atom (None: 1); `labels`: one per selected atom (None: one group
    of `n` atoms, or of len(weights)).  A pair with an empty group is NaN.  float64 on the host."""
    s = np.asarray(sab, np.float64)
    assert how in ("n", "w2")
    if labels is None:
        count = int(n) if n is not None else len(weights)
        lab = np.zeros(count, np.int64)
        G = 1
    else:
        lab = np.asarray(labels).astype(np.int64)
        G = int(ngroups) if ngroups is not None else int(lab.max()) + 1
    w = np.ones(lab.shape[0], np.float64) if weights is None else np.asarray(weights, np.float64)
    assert w.shape[0] == lab.shape[0], "one weight per selected atom"
    norm = np.bincount(lab, weights=(w * w if how == "w2" else np.ones_like(w)), minlength=G)
    pairs = sfactor_pairs(G)
    assert s.shape[0] == pairs.shape[0], "one row per pair a <= b"
    d = np.sqrt(norm[pairs[:, 0]] * norm[pairs[:, 1]])
    with np.errstate(divide="ignore", invalid="ignore"):
        return s / np.where(d > 0.0, d, np.nan).reshape((-1,) + (1,) * (s.ndim - 1))


def sfactor_intensity(sab_or_shell, form_factors):
    """I(q) = sum over the pairs a <= b of (2 - delta_ab) f_a(q) f_b(q) S_ab(q) from sab or shell [P, X] and the form
    factors [G] (constants) or [G, X] (one per lattice point or shell): how q-dependent form factors enter, since the call
    itself takes one weight per atom.  float64 on the host."""
    s = np.asarray(sab_or_shell, np.float64)
    f = np.asarray(form_factors, np.float64)
    if f.ndim == 1:
        f = f[:, None]
    pairs = sfactor_pairs(f.shape[0])
    assert s.ndim == 2 and s.shape[0] == pairs.shape[0], "one row per pair a <= b of the form factors' groups"
    mult = np.where(pairs[:, 0] == pairs[:, 1], 1.0, 2.0)[:, None]
    return (mult * f[pairs[:, 0]] * f[pairs[:, 1]] * s).sum(axis=0)


def sfactor_as_vectors(rho):
    """The series rho [F, G, Q, 2] (numpy or torch) as the block [F, G Q, 3] of (Re, Im, 0): vector_correlations(block,
    arange(G Q), mode="raw") then gives in c1_vec the intermediate scattering function F(q, tau) = <Re(rho(t) conj
    rho(t + tau))> of every group and lattice point (divide by N).  A NaN frame makes the series of its points bad."""
    F = rho.shape[0]
    if _is_torch(rho):
        import torch
        r = rho.reshape(F, -1, 2)
        return torch.cat([r, torch.zeros_like(r[..., :1])], dim=-1).contiguous()
    r = np.asarray(rho).reshape(F, -1, 2)
    return np.ascontiguousarray(np.concatenate([r, np.zeros_like(r[..., :1])], axis=-1))


def _sfactor_call(lib, fn, ctx, frames, grid, idx, weight, labels, ngroups, boxes, want, out, real):
    conv = _f32 if real == np.float32 else _f64
    fr, F, natoms, stride = _frame_block(frames, real)
    dev = _is_torch(fr)
    given_in = (idx, weight, labels, boxes)
    idx = _u64(idx); weight = conv(weight); labels = _u32(labels)
    box_stride = 0
    if boxes is not None:
        boxes = conv(boxes)
        if boxes.ndim == 2 and tuple(boxes.shape) == (3, 3):
            boxes = (boxes.T.contiguous() if _is_torch(boxes) else np.ascontiguousarray(boxes.T)).reshape(9)      # rows -> column-major
        if boxes.ndim == 2:
            assert tuple(boxes.shape) == (F, 9), "per-frame boxes are [F, 9], column-major"
            box_stride = 9
        else:
            assert tuple(boxes.shape) == (9,), "a box is [9] column-major or [3, 3]"
    n = natoms if idx is None else idx.shape[0]
    G = 1
    if labels is not None:
        assert labels.shape[0] == n, "one label per selected atom"
        G = int(ngroups) if ngroups is not None else (int(labels.max()) + 1 if n else 1)
    if weight is not None:
        assert weight.shape[0] == natoms, "one weight per atom"
    H, K, L = (int(v) for v in grid.hmax)
    Q = (H + 1) * (2 * K + 1) * (2 * L + 1)
    P = G * (G + 1) // 2
    ns = int(grid.nshells)
    names = ("rho", "frame_ok", "rho_mean", "sab", "shell", "shell_count")
    if want is None:
        want = ("frame_ok", "sab") + (("shell", "shell_count") if ns else ())
    want = tuple(want)
    assert all(nm in names for nm in want), "want holds names of StructureFactor"
    shapes = ((F, G, Q, 2), (F,), (G, Q, 2), (P, Q), (P, ns), (ns,))
    given = tuple(out[:6]) if out is not None else (None,) * 6
    res, rho_stride = [], 2 * Q
    for name, shape, g in zip(names, shapes, given):
        if name not in want:
            res.append(None)
            continue
        if dev:
            import torch
            dt = torch.int32 if name == "frame_ok" else torch.int64 if name == "shell_count" else fr.dtype
        else:
            dt = np.uint32 if name == "frame_ok" else np.uint64 if name == "shell_count" else real
        if g is not None:
            assert _is_torch(g) == dev and tuple(g.shape) == shape and g.dtype == dt
            if name == "rho" and F * G > 1:
                st = tuple(int(v) for v in g.stride()) if dev else tuple(v // g.dtype.itemsize for v in g.strides)
                assert st[3] == 1 and st[2] == 2 and st[1] >= 2 * Q and (F == 1 or st[0] == G * st[1]), "rho: rows (f, g) contiguous, one row stride"
                rho_stride = st[1] if G > 1 else (st[0] if F > 1 else 2 * Q)
            else:
                assert g.is_contiguous() if dev else g.flags.c_contiguous
            res.append(g)
        elif dev:
            res.append(torch.zeros(shape, dtype=dt, device=fr.device))
        else:
            res.append(np.zeros(shape, dt))
    addr = [None if r is None else (r.data_ptr() if dev else r.ctypes.data) for r in res]
    gs = _sfactor_struct(grid)
    fa = fr.data_ptr() if dev else fr.ctypes.data
    ia, k1 = _addr(idx); wa, k2 = _addr(weight); la, k3 = _addr(labels); ba, k4 = _addr(boxes)
    if dev:
        # torch made the outputs and any contiguous copy on ITS stream; the engine reads and writes on its own
        import torch
        torch.cuda.current_stream().synchronize()
    check(fn(ctx, fa, F, stride, natoms, ia, n, wa, la, G, ba, box_stride, C.addressof(gs), addr[0], rho_stride, addr[1], addr[2], addr[3],
             addr[4], addr[5]))
    if dev and (fr is not frames or any(a is not b for a, b in zip((idx, weight, labels, boxes), given_in))):
        # a temporary copy would go back to torch's allocator with the kernels that read it still enqueued: wait for them
        check(lib.molar_hip_synchronize(ctx))
    return StructureFactor(*res, grid)


MinDistances = collections.namedtuple("MinDistances", ["dist", "pair", "atom1", "near1", "atom2", "mat", "mat_mean", "mat_min", "mat_freq", "frame_ok", "nvalid"])
MINDIST_DIST, MINDIST_ATOM1, MINDIST_ATOM2, MINDIST_MAT = 1, 2, 4, 8          # MOLAR_HIP_MINDIST_*
_MINDIST_BITS = {"dist": 1, "pair": 1, "atom1": 2, "near1": 2, "atom2": 4, "mat": 8, "mat_mean": 8, "mat_min": 8, "mat_freq": 8, "frame_ok": 0, "nvalid": 0}


def _mindist_spec(pbc, same, exclude_same_group, cutoff, frame_block):
    sp = _lib.MindistSpec()
    sp.pbc = int(pbc)
    sp.same = int(bool(same))
    sp.exclude_same_group = int(bool(exclude_same_group))
    sp.frame_block = int(frame_block)
    sp.cutoff = float(cutoff)
    return sp


def mindist_plan(nframes, n1, n2=None, ngroups1=1, ngroups2=1, want=("dist", "pair"), same=False, frame_block=0):
    """(workspace_bytes, rows_per_wave, rows_per_block, cols_per_tile, col_splits, frame_block) of a min_distances call of
    these sizes asked for the outputs `want` (molar_hip_mindist_plan): the device workspace; the atoms of the row set a wave
    and a workgroup own; the columns a column split is a whole number of; the splits of the column set of the first pass;
    the frames walked at once.  The environment variables MOLAR_HIP_MINDIST_COL_SPLITS and MOLAR_HIP_MINDIST_FRAME_BLOCK
    override the last two, here and in the call.  A host function: no GPU is needed."""
    sp = _mindist_spec(7, same, False, 0.0, frame_block)
    outputs = 0
    for nm in want:
        outputs |= _MINDIST_BITS[nm]
    ws = C.c_size_t(0)
    u = [C.c_uint32(0) for _ in range(5)]
    check(_lib.load().molar_hip_mindist_plan(int(nframes), int(n1), int(n1 if n2 is None else n2), int(ngroups1), int(ngroups2), C.addressof(sp), outputs,
                                             C.addressof(ws), *(C.addressof(x) for x in u)))
    return (int(ws.value),) + tuple(int(x.value) for x in u)


def mindist_groups_from_resindex(resids, idx=None):
    """(labels uint32, ngroups) for min_distances from the residue column of a GRO topology (GroTopology.resids, one number
    per atom): a residue is a run of atoms with one number (the column wraps at 99999, so equal numbers far apart are
    different residues).  `idx`: the selection the labels are for (None: every atom); the residues the selection touches are
    numbered 0 .. ngroups - 1 in the order of the file."""
    r = np.asarray(resids).astype(np.int64).ravel()
    if r.shape[0] == 0:
        return np.zeros(0, np.uint32), 0
    residue = np.concatenate([[0], np.cumsum(r[1:] != r[:-1])])
    if idx is not None:
        residue = residue[np.asarray(idx).astype(np.int64)]
    present, labels = np.unique(residue, return_inverse=True)
    return labels.astype(np.uint32).reshape(-1), int(present.shape[0])


def _mindist_call(lib, fn, ctx, frames, idx1, idx2, labels1, labels2, ngroups1, ngroups2, boxes, pbc, same, exclude_same_group, cutoff, frame_block, want, out,
                  n1, n2, real):
    conv = _f32 if real == np.float32 else _f64
    fr, F, natoms, stride = _frame_block(frames, real)
    dev = _is_torch(fr)
    given_in = (idx1, idx2, labels1, labels2, boxes)
    idx1 = _u64(idx1); idx2 = _u64(idx2); labels1 = _u32(labels1); labels2 = _u32(labels2)
    same = bool(same)
    assert not (same and (idx2 is not None or labels2 is not None)), "same=True takes no second index or labels"
    box_stride = 0
    if boxes is not None:
        boxes = conv(boxes)
        if boxes.ndim == 2 and tuple(boxes.shape) == (3, 3):
            boxes = (boxes.T.contiguous() if _is_torch(boxes) else np.ascontiguousarray(boxes.T)).reshape(9)      # rows -> column-major
        if boxes.ndim == 2:
            assert tuple(boxes.shape) == (F, 9), "per-frame boxes are [F, 9], column-major"
            box_stride = 9
        else:
            assert tuple(boxes.shape) == (9,), "a box is [9] column-major or [3, 3]"
    else:
        pbc = 0
    n1 = int(idx1.shape[0]) if idx1 is not None else (natoms if n1 is None else int(n1))
    n2 = n1 if same else (int(idx2.shape[0]) if idx2 is not None else (natoms if n2 is None else int(n2)))
    G1 = G2 = 1
    if labels1 is not None:
        assert labels1.shape[0] == n1, "one label per atom of set 1"
        G1 = int(ngroups1) if ngroups1 is not None else (int(labels1.max()) + 1 if n1 else 1)
    if labels2 is not None:
        assert labels2.shape[0] == n2, "one label per atom of set 2"
        G2 = int(ngroups2) if ngroups2 is not None else (int(labels2.max()) + 1 if n2 else 1)
    if same:
        G2 = G1
    names = MinDistances._fields
    if want is None:
        want = ("dist", "pair", "frame_ok", "nvalid")
    want = tuple(want)
    assert all(nm in names for nm in want), "want holds names of MinDistances"
    assert not (same and "atom2" in want), "same=True: atom2 would be atom1"
    shapes = ((F,), (F, 2), (F, n1), (F, n1), (F, n2), (F, G1, G2), (G1, G2), (G1, G2), (G1, G2), (F,), (1,))
    given = tuple(out[:11]) if out is not None else (None,) * 11
    res, ld = [], {"atom1": n1, "near1": n1, "atom2": n2}
    for name, shape, g in zip(names, shapes, given):
        if name not in want:
            res.append(None)
            continue
        if dev:
            import torch
            dt = torch.int64 if name in ("pair", "near1", "nvalid") else torch.int32 if name in ("mat_freq", "frame_ok") else \
                torch.float64 if name == "mat_mean" else fr.dtype
        else:
            dt = np.uint64 if name in ("pair", "near1", "nvalid") else np.uint32 if name in ("mat_freq", "frame_ok") else \
                np.float64 if name == "mat_mean" else real
        if g is not None:
            assert _is_torch(g) == dev and tuple(g.shape) == shape and g.dtype == dt
            if name in ld and F > 1 and shape[1] > 0:
                st = tuple(int(v) for v in g.stride()) if dev else tuple(v // g.dtype.itemsize for v in g.strides)
                assert st[1] == 1 and st[0] >= shape[1], name + ": rows contiguous"
                ld[name] = st[0]
            else:
                assert g.is_contiguous() if dev else g.flags.c_contiguous
            res.append(g)
        elif dev:
            res.append(torch.zeros(shape, dtype=dt, device=fr.device))
        else:
            res.append(np.zeros(shape, dt))
    if "atom1" in want and "near1" in want:
        assert ld["atom1"] == ld["near1"], "atom1 and near1 share one row stride"
    ld1 = ld["atom1"] if "atom1" in want else ld["near1"]
    addr = [None if r is None else (r.data_ptr() if dev else r.ctypes.data) for r in res]
    sp = _mindist_spec(pbc, same, exclude_same_group, cutoff, frame_block)
    fa = fr.data_ptr() if dev else fr.ctypes.data
    i1, k1 = _addr(idx1); i2, k2 = _addr(idx2); l1, k3 = _addr(labels1); l2, k4 = _addr(labels2); ba, k5 = _addr(boxes)
    if dev:
        # torch made the outputs and any contiguous copy on ITS stream; the engine reads and writes on its own
        import torch
        torch.cuda.current_stream().synchronize()
    check(fn(ctx, fa, F, stride, natoms, i1, n1, l1, G1, i2, n2, l2, G2, ba, box_stride, C.addressof(sp), addr[0], addr[1], addr[2], addr[3], ld1, addr[4],
             ld["atom2"], addr[5], addr[6], addr[7], addr[8], addr[9], addr[10]))
    if dev and (fr is not frames or any(a is not b for a, b in zip((idx1, idx2, labels1, labels2, boxes), given_in))):
        # a temporary copy would go back to torch's allocator with the kernels that read it still enqueued: wait for them
        check(lib.molar_hip_synchronize(ctx))
    return MinDistances(*res)


VanHove = collections.namedtuple("VanHove", ["hist", "outside", "norigins", "nvalid", "bad", "edges"])
VanHovePlan = collections.namedtuple("VanHovePlan", ["workspace_bytes", "particles_per_wg", "origins_per_pass", "lag_tile", "on_chip", "lds_cells",
                                                     "pass_splits", "pairs_per_flush"])
VANHOVE_SIGNED = 1                                 # MOLAR_HIP_VANHOVE_SIGNED


def vanhove_plan(nframes, n, ngroups=1, nlags=1, nbins=1, ndims=3):
    """VanHovePlan of a van_hove call of these sizes (molar_hip_vanhove_plan): the device workspace and every launch-shape size
    the kernels branch on - the sorted particles a workgroup walks, the frames of origins of one pass, the lags of one tile,
    whether the counts go to the on-chip histogram (nbins <= lds_cells) and that limit, the workgroups that share the passes
    of one (particle chunk, lag tile), and the largest number of pairs an on-chip 32-bit cell can receive between two
    flushes (below 2^32).  ndims: the components that enter (1, 2 or 3).  A host function: no GPU is needed."""
    ws, ppf = C.c_size_t(0), C.c_uint64(0)
    u = [C.c_uint32(0) for _ in range(6)]
    check(_lib.load().molar_hip_vanhove_plan(int(nframes), int(n), int(ngroups), int(nlags), int(nbins), int(ndims), C.addressof(ws),
                                             *(C.addressof(x) for x in u), C.addressof(ppf)))
    return VanHovePlan(int(ws.value), *(int(x.value) for x in u), int(ppf.value))


def vanhove_lags(nframes, per_decade=8):
    """Log-spaced lags for van_hove: the distinct integers round(10^(k / per_decade)), k = 0, 1, ..., that stay below nframes,
    increasing, uint64 (1, 2, 3, ... at first, then `per_decade` lags per factor of ten).  One frame: the lag 0 alone."""
    F, per = int(nframes), int(per_decade)
    assert F >= 1 and per >= 1
    if F == 1:
        return np.zeros(1, np.uint64)
    k = np.arange(int(np.floor(np.log10(F - 1) * per)) + 2, dtype=np.float64)
    lags = np.unique(np.round(10.0 ** (k / per)).astype(np.int64))
    return lags[lags <= F - 1].astype(np.uint64)


def vanhove_edges(range, nbins):
    """The nbins + 1 bin edges of a van_hove histogram over the half-open range (lo, hi), float64."""
    lo, hi = float(range[0]), float(range[1])
    return lo + (hi - lo) * np.arange(int(nbins) + 1, dtype=np.float64) / int(nbins)


def vanhove_density(hist, nvalid, norigins, edges, ndims):
    """G_s(r, tau) as a probability density, float64 [G, L, nbins]: hist over the pairs nvalid[g] * norigins[l] and over the
    exact volume of the shell between the bin's edges - 4/3 pi (r1^3 - r0^3) for ndims = 3, pi (r1^2 - r0^2) for 2, r1 - r0
    for 1 (and for signed displacements).  Its integral over the shells is 1 minus the fraction of the pairs outside the
    range; NaN for a group without a valid particle."""
    h = np.asarray(hist, np.float64)
    e = np.asarray(edges, np.float64)
    pairs = np.asarray(nvalid, np.float64).reshape(-1, 1, 1) * np.asarray(norigins, np.float64).reshape(1, -1, 1)
    nd = int(ndims)
    assert nd in (1, 2, 3) and h.ndim == 3 and e.shape[0] == h.shape[2] + 1
    vol = e[1:] - e[:-1] if nd == 1 else np.pi * (e[1:] ** 2 - e[:-1] ** 2) if nd == 2 else 4.0 / 3.0 * np.pi * (e[1:] ** 3 - e[:-1] ** 3)
    with np.errstate(divide="ignore", invalid="ignore"):
        return h / pairs / vol


def bessel_j0(x):
    """J0(x) from its integral representation (1 / pi) int_0^pi cos(x sin theta) d theta by the trapezoid rule; the integrand
    is smooth and periodic, so the rule converges faster than any power once its panels outnumber |x|: float64 accuracy."""
    x = np.asarray(x, np.float64)
    flat = np.abs(x).reshape(-1)
    out = np.empty_like(flat)
    for s in np.arange(0, flat.shape[0], 4096):
        part = flat[s:s + 4096]
        m = int(np.ceil(part.max())) + 48 if part.size else 48
        theta = np.pi * np.arange(m + 1, dtype=np.float64) / m
        w = np.ones(m + 1)
        w[0] = w[-1] = 0.5
        out[s:s + 4096] = (np.cos(part[:, None] * np.sin(theta)[None, :]) * w).sum(axis=1) / m
    return out.reshape(x.shape)


def vanhove_fs(hist, outside, edges, q, ndims):
    """The isotropic self-intermediate scattering function F_s(q, tau) = <K(q r)> from a van_hove histogram, with r at the bin
    centres: K = sin(qr) / (qr) for ndims = 3, J0(qr) (bessel_j0) for 2, cos(qx) for 1 (signed or not).  hist [G, L, nbins],
    outside [G, L], q a number or [nq]; returns float64 [G, L, nq].  NaN where outside is not zero - a truncated distribution
    has no transform - and where no pair was counted.  Binning error: a value anywhere in a bin stands at its centre, which
    changes F_s by O((q dr)^2), dr the bin width: to leading order at most 5/24 (q dr)^2 (1/8 from the curvature of K inside
    a bin, 1/12 from the slope of the distribution across it)."""
    h = np.asarray(hist, np.float64)
    o = np.asarray(outside, np.float64)
    e = np.asarray(edges, np.float64)
    qs = np.atleast_1d(np.asarray(q, np.float64))
    nd = int(ndims)
    assert nd in (1, 2, 3) and h.ndim == 3 and e.shape[0] == h.shape[2] + 1 and qs.ndim == 1
    x = qs[:, None] * (0.5 * (e[1:] + e[:-1]))[None, :]                    # [nq, nbins]
    if nd == 1:
        K = np.cos(x)
    elif nd == 2:
        K = bessel_j0(x)
    else:
        K = np.sinc(x / np.pi)
    total = h.sum(axis=2)
    with np.errstate(divide="ignore", invalid="ignore"):
        fs = np.einsum("glb,qb->glq", h, K) / total[:, :, None]
    fs[(o != 0) | (total == 0)] = np.nan
    return fs


def _vanhove_call(lib, fn, ctx, traj, lags, range, nbins, idx, labels, ngroups, origin_stride, dims, signed, want, out, real):
    fr, F, natoms, stride = _frame_block(traj, real)
    dev = _is_torch(fr)
    given_in = (idx, labels, lags)
    idx = _u64(idx); labels = _u32(labels); lags = _u64(lags)
    assert lags.ndim == 1, "lags is a list"
    n = natoms if idx is None else int(idx.shape[0])
    L = int(lags.shape[0])
    G = 1
    if labels is not None:
        assert labels.shape[0] == n, "one label per selected particle"
        G = int(ngroups) if ngroups is not None else (int(labels.max()) + 1 if n else 1)
    nbins = int(nbins)
    lo, hi = float(range[0]), float(range[1])
    names = VanHove._fields[:5]
    want = names if want is None else tuple(want)
    assert all(nm in names for nm in want), "want holds names of VanHove"
    shapes = ((G, L, nbins), (G, L), (L,), (G,), (n,))
    given = tuple(out[:5]) if out is not None else (None,) * 5
    res = []
    for name, shape, g in zip(names, shapes, given):
        if name not in want:
            res.append(None)
            continue
        if dev:
            import torch
            dt = torch.int32 if name == "bad" else torch.int64
        else:
            dt = np.uint32 if name == "bad" else np.uint64
        if g is not None:
            assert _is_torch(g) == dev and tuple(g.shape) == shape and g.dtype == dt
            assert g.is_contiguous() if dev else g.flags.c_contiguous
            res.append(g)
        elif dev:
            res.append(torch.zeros(shape, dtype=dt, device=fr.device))
        else:
            res.append(np.zeros(shape, dt))
    addr = [None if r is None else (r.data_ptr() if dev else r.ctypes.data) for r in res]
    fa = fr.data_ptr() if dev else fr.ctypes.data
    ia, k1 = _addr(idx); la, k2 = _addr(labels); ga, k3 = _addr(lags)
    if dev:
        # torch made the outputs and any contiguous copy on ITS stream; the engine reads and writes on its own
        import torch
        torch.cuda.current_stream().synchronize()
    check(fn(ctx, fa, F, stride, natoms, ia, n, la, G, ga, L, int(origin_stride), int(dims), VANHOVE_SIGNED if signed else 0, lo, hi, nbins, *addr))
    if dev and (fr is not traj or any(_is_torch(a) and a is not b for a, b in zip((idx, labels, lags), given_in))):
        # a temporary copy would go back to torch's allocator with the kernels that read it still enqueued: wait for them
        check(lib.molar_hip_synchronize(ctx))
    edges = vanhove_edges((lo, hi), nbins) if nbins >= 1 and np.isfinite(lo) and np.isfinite(hi) else None
    return VanHove(*res, edges)


def _vanhove_frames_call(msd, van_hove, frames, lags, range, nbins, idx, mass, boxes, pbc, groups, ref_idx, labels, ngroups, origin_stride, dims, signed, want, out):
    disp = msd(frames, idx=idx, mass=mass, boxes=boxes, pbc=pbc, groups=groups, ref_idx=ref_idx, disp=True, msd=False, m4=False).disp
    return van_hove(disp, lags, range, nbins, labels=labels, ngroups=ngroups, origin_stride=origin_stride, dims=dims, signed=signed, want=want, out=out)


Fluctuations = collections.namedtuple("Fluctuations", ["mean", "rmsf", "cov", "fit"])


def _fluct_call(lib, fn, ctx, frames, idx, mass, ref, fit, iterations, cov, fit_out, out, real):
    conv = _f32 if real == np.float32 else _f64
    fr, F, natoms, stride = _frame_block(frames, real)
    dev = _is_torch(fr)
    idx_in, mass_in, ref_in = idx, mass, ref
    idx = _u64(idx); mass = conv(mass); ref = conv(ref)
    n = natoms if idx is None else idx.shape[0]
    if mass is not None:
        assert mass.shape[0] == natoms, "one mass per atom"
    if ref is not None:
        assert tuple(ref.shape) == (n, 3), "ref holds the selected atoms, [n, 3]"
    want = (True, True, bool(cov), bool(fit_out))
    shapes = ((n, 3), (n,), (3 * n, 3 * n), (F, 13))
    given = tuple(out) if out is not None else (None,) * 4
    res = []
    for w, shape, g in zip(want, shapes, given):
        if not w:
            res.append(None)
        elif g is not None:
            assert _is_torch(g) == dev and tuple(g.shape) == shape
            assert (g.dtype == fr.dtype and g.is_contiguous()) if dev else (g.dtype == real and g.flags.c_contiguous)
            res.append(g)
        elif dev:
            import torch
            res.append(torch.zeros(shape, dtype=fr.dtype, device=fr.device))
        else:
            res.append(np.zeros(shape, real))
    addr = [None if r is None else (r.data_ptr() if dev else r.ctypes.data) for r in res]
    fa = fr.data_ptr() if dev else fr.ctypes.data
    ia, k1 = _addr(idx); ma, k2 = _addr(mass); ra, k3 = _addr(ref)
    if dev:
        # torch made the outputs and any contiguous copy on ITS stream; the engine reads and writes on its own
        import torch
        torch.cuda.current_stream().synchronize()
    check(fn(ctx, fa, F, stride, natoms, ia, n, ma, ra, 1 if fit else 0, int(iterations), addr[0], addr[1], addr[2], 3 * n, addr[3]))
    if dev and (fr is not frames or idx is not idx_in or mass is not mass_in or ref is not ref_in):
        # a temporary copy would go back to torch's allocator with the kernels that read it still enqueued: wait for them
        check(lib.molar_hip_synchronize(ctx))
    return Fluctuations(*res)


def _f64(x):
    if x is None:
        return None
    if _is_torch(x):
        import torch
        assert x.dtype == torch.float64
        return x.contiguous()
    return np.ascontiguousarray(x, dtype=np.float64)


class MeasureF64:
    """The Measure / Modify methods for MolAR's `f64` feature (Float = f64, molar/src/aliases.rs:10-13) on
    an Engine's context: float64 coordinates and masses (numpy or torch CUDA), float64 results.  Same argument meaning
    as the Engine methods of the same name.  (The f64 search: Engine.search_f64, within_set_f64, search_connectivity_f64.)"""

    def __init__(self, engine: "Engine"):
        self.eng, self.lib, self.ctx = engine, engine.lib, engine.ctx

    @staticmethod
    def _sel(xyz, idx):
        xyz = _f64(xyz); idx = _u64(idx)
        xa, k1 = _addr(xyz); ia, k2 = _addr(idx)
        natoms = xyz.shape[0] if xyz.ndim == 2 else xyz.shape[0] // 3
        return xa, natoms, ia, (0 if idx is None else idx.shape[0]), (k1, k2)

    def center_of_geometry(self, xyz, idx=None):
        a = self._sel(xyz, idx)
        out = np.zeros(3, np.float64)
        check(self.lib.molar_hip_center_of_geometry_f64(self.ctx, *a[:4], out.ctypes.data))
        return out

    def center_of_mass(self, xyz, mass, idx=None):
        a = self._sel(xyz, idx)
        mass = _f64(mass); ma, km = _addr(mass)
        out = np.zeros(3, np.float64)
        check(self.lib.molar_hip_center_of_mass_f64(self.ctx, *a[:4], ma, out.ctypes.data))
        return out

    def gyration(self, xyz, mass, idx=None):
        a = self._sel(xyz, idx)
        mass = _f64(mass); ma, km = _addr(mass)
        out = C.c_double(0)
        check(self.lib.molar_hip_gyration_f64(self.ctx, *a[:4], ma, C.byref(out)))
        return float(out.value)

    def rmsd(self, xyz1, xyz2, idx1=None, idx2=None):
        a1 = self._sel(xyz1, idx1); a2 = self._sel(xyz2, idx2)
        out = C.c_double(0)
        check(self.lib.molar_hip_rmsd_f64(self.ctx, *a1[:4], *a2[:4], C.byref(out)))
        return float(out.value)

    def rmsd_mw(self, xyz1, mass1, xyz2, idx1=None, idx2=None):
        a1 = self._sel(xyz1, idx1); a2 = self._sel(xyz2, idx2)
        mass1 = _f64(mass1); ma, km = _addr(mass1)
        out = C.c_double(0)
        check(self.lib.molar_hip_rmsd_mw_f64(self.ctx, *a1[:4], ma, *a2[:4], C.byref(out)))
        return float(out.value)

    def fit_transform(self, xyz1, mass1, xyz2, mass2, idx1=None, idx2=None, at_origin=False):
        """(R, t) with p -> R @ p + t."""
        a1 = self._sel(xyz1, idx1); a2 = self._sel(xyz2, idx2)
        mass1 = _f64(mass1); m1, k1 = _addr(mass1)
        mass2 = _f64(mass2); m2, k2 = _addr(mass2)
        R = np.zeros(9, np.float64); t = np.zeros(3, np.float64)
        check(self.lib.molar_hip_fit_transform_f64(self.ctx, *a1[:4], m1, *a2[:4], m2, 1 if at_origin else 0,
                                                   R.ctypes.data, t.ctypes.data))
        return R.reshape(3, 3).T.copy(), t

    @staticmethod
    def _box9(box):
        """box: 3x3 with COLUMNS = box vectors (PeriodicBox::from_matrix), float64."""
        b9 = np.ascontiguousarray(np.asarray(box, np.float64).reshape(3, 3).T).reshape(9)
        return b9.ctypes.data, b9

    def center_of_geometry_pbc(self, xyz, box, dims=PBC_FULL, idx=None):
        a = self._sel(xyz, idx); ba, kb = self._box9(box)
        out = np.zeros(3, np.float64)
        check(self.lib.molar_hip_center_of_geometry_pbc_f64(self.ctx, *a[:4], ba, pbc_mask(dims), out.ctypes.data))
        return out

    def center_of_mass_pbc(self, xyz, mass, box, dims=PBC_FULL, idx=None):
        a = self._sel(xyz, idx); ba, kb = self._box9(box)
        mass = _f64(mass); ma, km = _addr(mass)
        out = np.zeros(3, np.float64)
        check(self.lib.molar_hip_center_of_mass_pbc_f64(self.ctx, *a[:4], ma, ba, pbc_mask(dims), out.ctypes.data))
        return out

    def gyration_pbc(self, xyz, mass, box, idx=None):
        a = self._sel(xyz, idx); ba, kb = self._box9(box)
        mass = _f64(mass); ma, km = _addr(mass)
        out = C.c_double(0)
        check(self.lib.molar_hip_gyration_pbc_f64(self.ctx, *a[:4], ma, ba, C.byref(out)))
        return float(out.value)

    def unwrap_simple(self, xyz, box, dims=PBC_FULL, idx=None):
        if not _is_torch(xyz):
            assert xyz.dtype == np.float64 and xyz.flags.c_contiguous, "unwrap_simple works in place"
        a = self._sel(xyz, idx); ba, kb = self._box9(box)
        check(self.lib.molar_hip_unwrap_simple_f64(self.ctx, *a[:4], ba, pbc_mask(dims)))

    def unwrap_connectivity(self, xyz, box, cutoff, dims=PBC_FULL, idx=None):
        """Modify::unwrap_connectivity_dim (modify.rs:72-131) in place with Float = f64 (molar_hip_unwrap_connectivity_f64):
        f64 neighbour search with local ids on the GPU, adjacency in pair order, the reference's stack walk inside the
        library.  Returns what Engine.unwrap_connectivity returns: the list of groups of LOCAL indices."""
        if not _is_torch(xyz):
            assert xyz.dtype == np.float64 and xyz.flags.c_contiguous, "unwrap_connectivity works in place"
        if idx is not None and len(idx) == 0:      # (a NULL index means "all atoms" to the C ABI: never pass an empty one as NULL)
            raise ValueError("unwrap_connectivity: empty selection")
        xa, na, ia, n, k = self._sel(xyz, idx)
        nsel = n if idx is not None else na
        ba, kb = self._box9(box) if box is not None else (None, None)      # no box: the library's NO_PBC
        goff = np.zeros(nsel + 1, np.uint64); gids = np.zeros(max(nsel, 1), np.uint64)
        ng = C.c_size_t(0)
        check(self.lib.molar_hip_unwrap_connectivity_f64(self.ctx, xa, na, ia, n, ba, float(cutoff), pbc_mask(dims), goff.ctypes.data,
                                                         gids.ctypes.data, C.byref(ng)))
        return [gids[int(goff[g]):int(goff[g + 1])].copy() for g in range(int(ng.value))]

    def fit_rmsd_batch(self, frames, mass, ref_xyz, idx=None, ref_idx=None, apply=True):
        """frames: float64 [F, natoms, 3] (numpy, modified in place if apply; or torch CUDA tensor).
        Returns dict(rmsd[F], R[F,3,3], t[F,3], com[F,3], gyration[F]) in float64."""
        if not _is_torch(frames):
            assert frames.dtype == np.float64 and frames.flags.c_contiguous
        else:
            import torch
            assert frames.dtype == torch.float64 and frames.is_contiguous()
        F, natoms = frames.shape[0], frames.shape[1]
        fa, kf = _addr(frames)
        idx = _u64(idx); ref_idx = _u64(ref_idx) if ref_idx is not None else idx
        ia, ki = _addr(idx); ra, kr = _addr(ref_idx)
        n = 0 if idx is None else idx.shape[0]
        mass = _f64(mass); ma, km = _addr(mass)
        ref_xyz = _f64(ref_xyz); xa, kx = _addr(ref_xyz)
        ref_natoms = ref_xyz.shape[0] if ref_xyz.ndim == 2 else ref_xyz.shape[0] // 3
        rm = np.zeros(F, np.float64); R = np.zeros((F, 9), np.float64); t = np.zeros((F, 3), np.float64)
        com = np.zeros((F, 3), np.float64); gy = np.zeros(F, np.float64)
        check(self.lib.molar_hip_fit_rmsd_batch_f64(self.ctx, fa, F, natoms, ia, n, ma, xa, ref_natoms, ra,
                                                    1 if apply else 0, rm.ctypes.data, R.ctypes.data, t.ctypes.data,
                                                    com.ctypes.data, gy.ctypes.data))
        return dict(rmsd=rm, R=R.reshape(F, 3, 3).transpose(0, 2, 1).copy(), t=t, com=com, gyration=gy)

    def rmsd_matrix(self, frames, idx=None, mass=None, frames2=None, fit=True, out=None):
        """Engine.rmsd_matrix on float64 frames and masses (molar_hip_rmsd_matrix_f64): float64 results."""
        return _rmsd_matrix_call(self.lib, self.lib.molar_hip_rmsd_matrix_f64, self.ctx, frames, idx, mass, frames2, fit, out, np.float64)

    def fluctuations(self, frames, idx=None, mass=None, ref=None, fit=True, iterations=0, cov=False, fit_out=False, out=None):
        """Engine.fluctuations on float64 frames, masses and reference (molar_hip_fluct_f64): float64 results."""
        return _fluct_call(self.lib, self.lib.molar_hip_fluct_f64, self.ctx, frames, idx, mass, ref, fit, iterations, cov, fit_out, out, np.float64)

    def msd(self, frames, idx=None, mass=None, boxes=None, pbc=7, groups=None, ref_idx=None, max_lag=None, origin_stride=1, dims=7,
            m4=True, per_particle=False, disp=False, msd=True, out=None):
        """Engine.msd on float64 frames, masses and boxes (molar_hip_msd_f64): float64 results."""
        return _msd_call(self.lib, self.lib.molar_hip_msd_f64, self.ctx, frames, idx, mass, boxes, pbc, groups, ref_idx, max_lag, origin_stride,
                         dims, msd, m4, per_particle, disp, out, np.float64)

    def internal_coords(self, frames, tuples, kind=None, labels=None, ngroups=None, boxes=None, pbc=7, nbins=0, range=None, pairs=None,
                        pair_labels=None, npair_groups=None, map_bins=0, want=None, out=None):
        """Engine.internal_coords on float64 frames and boxes (molar_hip_intcoord_f64): float64 results."""
        return _intcoord_call(self.lib, self.lib.molar_hip_intcoord_f64, self.ctx, frames, tuples, kind, labels, ngroups, boxes, pbc, nbins, range,
                              pairs, pair_labels, npair_groups, map_bins, want, out, np.float64)

    def vector_correlations(self, frames, tuples, kind=None, labels=None, ngroups=None, boxes=None, pbc=7, mode="unit", dims=7, max_lag=None,
                            origin_stride=1, want=None, out=None):
        """Engine.vector_correlations on float64 frames and boxes (molar_hip_tcf_f64): float64 results."""
        return _tcf_call(self.lib, self.lib.molar_hip_tcf_f64, self.ctx, frames, tuples, kind, labels, ngroups, boxes, pbc, mode, dims, max_lag,
                         origin_stride, want, out, np.float64)

    def density(self, frames, grid, idx=None, weight=None, labels=None, ngroups=None, boxes=None, pbc=7, centre_idx=None,
                centre_weight=None, want=None, out=None):
        """Engine.density on float64 frames, weights and boxes (molar_hip_density_f64): float64 results."""
        return _density_call(self.lib, self.lib.molar_hip_density_f64, self.ctx, frames, grid, idx, weight, labels, ngroups, boxes, pbc,
                             centre_idx, centre_weight, want, out, np.float64)

    def structure_factor(self, frames, grid, idx=None, weight=None, labels=None, ngroups=None, boxes=None, want=None, out=None):
        """Engine.structure_factor on float64 frames, weights and boxes (molar_hip_sfactor_f64): float64 results."""
        return _sfactor_call(self.lib, self.lib.molar_hip_sfactor_f64, self.ctx, frames, grid, idx, weight, labels, ngroups, boxes, want, out, np.float64)

    def min_distances(self, frames, idx1=None, idx2=None, labels1=None, labels2=None, ngroups1=None, ngroups2=None, boxes=None, pbc=7, same=False,
                      exclude_same_group=False, cutoff=0.0, frame_block=0, want=None, out=None, n1=None, n2=None):
        """Engine.min_distances on float64 frames and boxes (molar_hip_mindist_f64): float64 results."""
        return _mindist_call(self.lib, self.lib.molar_hip_mindist_f64, self.ctx, frames, idx1, idx2, labels1, labels2, ngroups1, ngroups2, boxes, pbc,
                             same, exclude_same_group, cutoff, frame_block, want, out, n1, n2, np.float64)

    def van_hove(self, traj, lags, range, nbins, idx=None, labels=None, ngroups=None, origin_stride=1, dims=7, signed=False, want=None, out=None):
        """Engine.van_hove for traj [F, natoms, 3] float64 (molar_hip_vanhove_f64); the counts are integers either way."""
        return _vanhove_call(self.lib, self.lib.molar_hip_vanhove_f64, self.ctx, traj, lags, range, nbins, idx, labels, ngroups, origin_stride, dims, signed, want,
                             out, np.float64)

    def van_hove_frames(self, frames, lags, range, nbins, idx=None, boxes=None, pbc=7, mass=None, groups=None, ref_idx=None, labels=None, ngroups=None,
                        origin_stride=1, dims=7, signed=False, want=None, out=None):
        """Engine.van_hove_frames for frames [F, natoms, 3] float64: self.msd, then self.van_hove on its `disp`."""
        return _vanhove_frames_call(self.msd, self.van_hove, frames, lags, range, nbins, idx, mass, boxes, pbc, groups, ref_idx, labels, ngroups,
                                    origin_stride, dims, signed, want, out)

    def sasa(self, xyz, vdw, idx=None, probe=0.14, npoints=960, want_exposed=False):
        """Engine.sasa on float64 coordinates and radii (molar_hip_sasa_f64): every operation of the two compares in f64."""
        return _sasa_call(self.lib.molar_hip_sasa_f64, self.ctx, _f64(xyz), _f64(vdw), _sel(idx), C.c_double(probe), npoints,
                          want_exposed, np.float64)

    def sasa_vol(self, xyz, vdw, idx=None, probe=0.14, npoints=960, want_exposed=False):
        """Engine.sasa_vol on float64 coordinates and radii (molar_hip_sasa_vol_f64): compares, cuts and division in f64."""
        return _sasa_call(self.lib.molar_hip_sasa_vol_f64, self.ctx, _f64(xyz), _f64(vdw), _sel(idx), C.c_double(probe), npoints,
                          want_exposed, np.float64, want_volumes=True)

    def min_max(self, xyz, idx=None):
        a = self._sel(xyz, idx)
        lo = np.zeros(3, np.float64); hi = np.zeros(3, np.float64)
        check(self.lib.molar_hip_min_max_f64(self.ctx, *a[:4], lo.ctypes.data, hi.ctypes.data))
        return lo, hi

    def inertia(self, xyz, mass, idx=None, box=None):
        """(moments[3] ascending, axes 3x3 with axes as columns, raw tensor 3x3); inertia_pbc with a box."""
        a = self._sel(xyz, idx)
        mass = _f64(mass); ma, km = _addr(mass)
        mom = np.zeros(3, np.float64); axes = np.zeros(9, np.float64); tens = np.zeros(9, np.float64)
        if box is None:
            check(self.lib.molar_hip_inertia_f64(self.ctx, *a[:4], ma, mom.ctypes.data, axes.ctypes.data, tens.ctypes.data))
        else:
            ba, kb = self._box9(box)
            check(self.lib.molar_hip_inertia_pbc_f64(self.ctx, *a[:4], ma, ba, mom.ctypes.data, axes.ctypes.data,
                                                     tens.ctypes.data))
        return mom, axes.reshape(3, 3).T.copy(), tens.reshape(3, 3).T.copy()

    def translate(self, xyz, shift, idx=None):
        if not _is_torch(xyz):
            assert xyz.dtype == np.float64 and xyz.flags.c_contiguous, "translate works in place"
        a = self._sel(xyz, idx)
        sh = np.ascontiguousarray(shift, np.float64)
        check(self.lib.molar_hip_translate_f64(self.ctx, *a[:4], sh.ctypes.data))

    def lipid_tail_order(self, xyz, tails, order_type, normals, bond_orders):
        """Batched Measure::lipid_tail_order (measure.rs:270-422) in f64; arguments as Engine.lipid_tail_order."""
        xyz = _f64(xyz)
        xa, kx = _addr(xyz)
        lens = np.array([len(t) for t in tails], dtype=np.uint64)
        toff = np.concatenate([[0], np.cumsum(lens)]).astype(np.uint64)
        idx = np.ascontiguousarray(np.concatenate([np.asarray(t, np.uint64) for t in tails]))
        nl = [np.asarray(n, np.float64).reshape(-1, 3) for n in normals]
        noff = np.concatenate([[0], np.cumsum([len(n) for n in nl])]).astype(np.uint64)
        nrm = np.ascontiguousarray(np.concatenate(nl))
        bo = np.ascontiguousarray(np.concatenate([np.asarray(b, np.uint8) for b in bond_orders])) if bond_orders is not None else None
        if bo is not None and len(bo) != int(toff[-1]) - len(tails):
            raise MolarHipError(9, "for N tail carbons # of bond orders should be N-1")       # LipidOrderError::BondOrderCount
        nout = max(int(toff[-1]) - 2 * len(tails), 0)
        out = np.zeros(max(nout, 1), np.float64)
        check(self.lib.molar_hip_lipid_tail_order_f64(self.ctx, xa, xyz.shape[0], idx.ctypes.data, toff.ctypes.data, len(tails),
                                                      int(order_type), nrm.ctypes.data, noff.ctypes.data,
                                                      None if bo is None else bo.ctypes.data, out.ctypes.data))
        res, pos = [], 0
        for n in lens:
            res.append(out[pos:pos + int(n) - 2].copy()); pos += int(n) - 2
        return res

    def lipid_tail_order_csr(self, xyz, idx, tail_offsets, order_type, normals, normal_offsets, bond_orders):
        """lipid_tail_order in f64 with the CSR arrays prepared by the caller (as Engine.lipid_tail_order_csr)."""
        xyz = _f64(xyz)
        xa, kx = _addr(xyz)
        idx = _u64(idx); tail_offsets = np.ascontiguousarray(tail_offsets, np.uint64)
        normal_offsets = np.ascontiguousarray(normal_offsets, np.uint64)
        normals = np.ascontiguousarray(normals, np.float64)
        if not _is_torch(bond_orders):
            bond_orders = np.ascontiguousarray(bond_orders, np.uint8)
        ia, ki = _addr(idx); ba, kb = _addr(bond_orders)
        K = len(tail_offsets) - 1
        nout = int(tail_offsets[-1]) - 2 * K
        out = np.zeros(max(nout, 1), np.float64)
        natoms = xyz.shape[0] if xyz.ndim == 2 else xyz.shape[0] // 3
        check(self.lib.molar_hip_lipid_tail_order_f64(self.ctx, xa, natoms, ia, tail_offsets.ctypes.data, K, int(order_type),
                                                      normals.ctypes.data, normal_offsets.ctypes.data, ba, out.ctypes.data))
        return out[:nout]

    def rotate(self, xyz, unit_axis, angle, idx=None):
        if not _is_torch(xyz):
            assert xyz.dtype == np.float64 and xyz.flags.c_contiguous, "rotate works in place"
        a = self._sel(xyz, idx)
        ax = np.ascontiguousarray(unit_axis, np.float64)
        check(self.lib.molar_hip_rotate_f64(self.ctx, *a[:4], ax.ctypes.data, float(angle)))

    def principal_transform(self, xyz, mass, idx=None, box=None):
        """(R, t) of Translation(cm) * Rotation(axes^-1) * Translation(-cm); principal_transform_pbc with a box."""
        a = self._sel(xyz, idx)
        mass = _f64(mass); ma, km = _addr(mass)
        ba, kb = self._box9(box) if box is not None else (None, None)
        R = np.zeros(9, np.float64); t = np.zeros(3, np.float64)
        check(self.lib.molar_hip_principal_transform_f64(self.ctx, *a[:4], ma, ba, R.ctypes.data, t.ctypes.data))
        return R.reshape(3, 3).T.copy(), t

    def apply_transform(self, xyz, R, t, idx=None):
        """In place on xyz (numpy float64 C-contiguous array or torch CUDA tensor)."""
        if not _is_torch(xyz):
            assert xyz.dtype == np.float64 and xyz.flags.c_contiguous, "apply_transform works in place"
        a = self._sel(xyz, idx)
        R9 = np.ascontiguousarray(np.asarray(R, np.float64).reshape(3, 3).T).reshape(9)
        t3 = np.ascontiguousarray(t, np.float64)
        check(self.lib.molar_hip_apply_transform_f64(self.ctx, *a[:4], R9.ctypes.data, t3.ctypes.data))

    def center_batch(self, xyz, idx, offsets, mass=None):
        """Centres of K CSR selections (idx, offsets[K+1]) in f64: center_of_mass if `mass` is given, else
        center_of_geometry, the reference's serial sums.  Returns float64 [K,3]."""
        xyz = _f64(xyz); idx = _u64(idx); offsets = _u64(offsets); mass = _f64(mass)
        xa, k1 = _addr(xyz); ia, k2 = _addr(idx); oa, k3 = _addr(offsets); ma, k4 = _addr(mass)
        K = offsets.shape[0] - 1
        out = np.zeros((K, 3), np.float64)
        natoms = xyz.shape[0] if xyz.ndim == 2 else xyz.shape[0] // 3
        check(self.lib.molar_hip_center_batch_f64(self.ctx, xa, natoms, ia, oa, K, ma, out.ctypes.data))
        return out

    def unwrap_simple_batch(self, xyz, idx, offsets, box, dims=PBC_FULL):
        """unwrap_simple on each of K CSR selections in f64, in place (numpy float64 C-contiguous or torch CUDA float64)."""
        if not _is_torch(xyz):
            assert xyz.dtype == np.float64 and xyz.flags.c_contiguous, "unwrap_simple_batch works in place"
        else:
            import torch
            assert xyz.dtype == torch.float64 and xyz.is_contiguous(), "unwrap_simple_batch works in place"
        idx = _u64(idx); offsets = _u64(offsets)
        xa, k1 = _addr(xyz); ia, k2 = _addr(idx); oa, k3 = _addr(offsets)
        ba, kb = self._box9(box)
        natoms = xyz.shape[0] if xyz.ndim == 2 else xyz.shape[0] // 3
        check(self.lib.molar_hip_unwrap_simple_batch_f64(self.ctx, xa, natoms, ia, oa, offsets.shape[0] - 1, ba,
                                                         pbc_mask(dims)))
        return xyz

    def membrane_smooth(self, box, state, patch_offsets, patch_ids):
        """One iteration of Membrane::smooth (molar_membrane/src/lib.rs:661-812) in f64.  `state`: a float64 dict of
        new_membrane_state(..., dtype=np.float64), updated IN PLACE as by Engine.membrane_smooth."""
        if state["head_markers"].dtype != np.float64:
            raise TypeError("MeasureF64.membrane_smooth takes a float64 state (new_membrane_state(..., dtype=np.float64))")
        pb = box.get_matrix() if isinstance(box, PeriodicBox) else box
        ba, kb = self._box9(pb)
        return _membrane_smooth_call(self.lib.molar_hip_membrane_smooth_f64, self.ctx, ba, state, patch_offsets, patch_ids,
                                     np.float64)


_MEMBRANE_FIELDS = ("head_markers", "normals", "valid", "quad_coefs", "mean_curv", "gauss_curv", "princ_curvs",
                    "princ_dirs", "area", "nvert", "neib_ids", "voro_vertexes", "fitted_patch_points")


class _MembranePatches(C.Structure):     # molar_hip_membrane_patches
    _fields_ = [("nlipids", C.c_size_t), ("patch_offsets", C.c_void_p), ("patch_ids", C.c_void_p)]


class _MembraneState(C.Structure):       # molar_hip_membrane_state
    _fields_ = [(k, C.c_void_p) for k in _MEMBRANE_FIELDS]


def new_membrane_state(head_markers, normals, valid=None, npatch_entries=0, dtype=np.float32):
    """Per-lipid state with the defaults of Membrane::new (molar_membrane/src/lib.rs:152-177); dtype np.float32 (the
    engine's f32 pass) or np.float64 (MeasureF64.membrane_smooth)."""
    f = np.dtype(dtype)
    if f not in (np.dtype(np.float32), np.dtype(np.float64)):
        raise TypeError(f"membrane state dtype must be float32 or float64, not {f}")
    head = np.array(head_markers, f, order="C").reshape(-1, 3)
    K = len(head)
    slots = max(npatch_entries + 4 * K, 1)
    return dict(
        head_markers=head, normals=np.array(normals, f, order="C").reshape(K, 3),
        valid=np.ones(K, np.uint8) if valid is None else np.array(valid, np.uint8, order="C"),
        quad_coefs=np.zeros((K, 6), f), mean_curv=np.full(K, -100.0, f),
        gauss_curv=np.full(K, -100.0, f), princ_curvs=np.zeros((K, 2), f),
        princ_dirs=np.zeros((K, 2, 3), f), area=np.zeros(K, f), nvert=np.zeros(K, np.uint32),
        neib_ids=np.zeros(slots, np.uint64), voro_vertexes=np.zeros((slots, 3), f),
        fitted_patch_points=np.zeros((max(npatch_entries, 1), 3), f))


def _membrane_smooth_call(fn, ctx, box9_addr, state, patch_offsets, patch_ids, real):
    """The call behind Engine.membrane_smooth (f32) and MeasureF64.membrane_smooth (f64): re-slots the state when the patch
    structure changed, then one smoothing pass in place."""
    po = _u64(patch_offsets); pi = _u64(patch_ids)
    K = len(po) - 1
    E = int(po[-1]); slots = E + 4 * K
    st = state
    if st["neib_ids"].shape[0] != max(slots, 1):                       # patch structure changed: re-slot
        st["neib_ids"] = np.zeros(max(slots, 1), np.uint64)
        st["voro_vertexes"] = np.zeros((max(slots, 1), 3), real)
        st["fitted_patch_points"] = np.zeros((max(E, 1), 3), real)
        st["nvert"][:] = 0
    for k in _MEMBRANE_FIELDS:
        if k not in ("valid", "nvert", "neib_ids") and st[k].dtype != real:
            raise TypeError(f"membrane state: {k} is {st[k].dtype}, the pass works in {np.dtype(real)}")
    P = _MembranePatches(K, po.ctypes.data, pi.ctypes.data if E else None)
    S = _MembraneState(*[st[k].ctypes.data for k in _MEMBRANE_FIELDS])
    check(fn(ctx, C.byref(P), box9_addr, C.byref(S)))
    return st


class MembranePlan:
    """molar_hip_membrane_plan: one frame of Membrane::compute (molar_membrane/src/lib.rs:410-454) per begin/end pair,
    chained on the engine's stream without a host round trip inside; two frames may be in flight.  `valid` is carried
    from frame to frame on the device like LipidMolecule::valid."""

    # (dtype, shape as a function of K, E, slots, norder)
    _SHAPES = {
        "head": (np.float32, lambda K, E, S, N: (K, 3)), "mid": (np.float32, lambda K, E, S, N: (K, 3)),
        "tail": (np.float32, lambda K, E, S, N: (K, 3)), "patch_offsets": (np.uint64, lambda K, E, S, N: (K + 1,)),
        "patch_ids": (np.uint64, lambda K, E, S, N: (E,)), "initial_normals": (np.float32, lambda K, E, S, N: (K, 3)),
        "valid": (np.uint8, lambda K, E, S, N: (K,)), "smoothed_head": (np.float32, lambda K, E, S, N: (K, 3)),
        "normals": (np.float32, lambda K, E, S, N: (K, 3)), "quad_coefs": (np.float32, lambda K, E, S, N: (K, 6)),
        "mean_curv": (np.float32, lambda K, E, S, N: (K,)), "gauss_curv": (np.float32, lambda K, E, S, N: (K,)),
        "princ_curvs": (np.float32, lambda K, E, S, N: (K, 2)), "princ_dirs": (np.float32, lambda K, E, S, N: (K, 2, 3)),
        "area": (np.float32, lambda K, E, S, N: (K,)), "nvert": (np.uint32, lambda K, E, S, N: (K,)),
        "neib_ids": (np.uint64, lambda K, E, S, N: (S,)), "voro_vertexes": (np.float32, lambda K, E, S, N: (S, 3)),
        "fitted_patch_points": (np.float32, lambda K, E, S, N: (E, 3)), "order": (np.float32, lambda K, E, S, N: (N,)),
    }

    def __init__(self, engine, natoms, lipid_idx, lipid_off, marker_idx, marker_off, masses, tail_idx, tail_off, tail_lipid,
                 tail_bonds, cutoff, order_type, max_smooth_iter=1, unwrap=True, global_normal=None):
        self.eng = engine
        self.lib = engine.lib
        keep = [np.ascontiguousarray(lipid_idx, np.uint64), np.ascontiguousarray(lipid_off, np.uint64),
                np.ascontiguousarray(marker_idx, np.uint64), np.ascontiguousarray(marker_off, np.uint64),
                np.ascontiguousarray(masses, np.float32), np.ascontiguousarray(tail_idx, np.uint64),
                np.ascontiguousarray(tail_off, np.uint64), np.ascontiguousarray(tail_lipid, np.uint32),
                None if tail_bonds is None else np.ascontiguousarray(tail_bonds, np.uint8)]
        d = MembraneDesc()
        d.natoms = int(natoms); d.nlipids = len(keep[1]) - 1
        d.lipid_idx, d.lipid_offsets, d.marker_idx, d.marker_offsets, d.masses = (a.ctypes.data for a in keep[:5])
        d.ntails = len(keep[6]) - 1
        d.tail_idx, d.tail_offsets, d.tail_lipid = keep[5].ctypes.data, keep[6].ctypes.data, keep[7].ctypes.data
        d.tail_bonds = None if keep[8] is None else keep[8].ctypes.data
        d.cutoff = float(cutoff); d.order_type = int(order_type); d.max_smooth_iter = int(max_smooth_iter); d.unwrap = int(bool(unwrap))
        d.use_global_normal = int(global_normal is not None)
        g = np.zeros(3, np.float32) if global_normal is None else np.asarray(global_normal, np.float32).reshape(3)
        d.global_normal[:] = [float(v) for v in g]
        self.K = int(d.nlipids)
        self.norder = int(keep[6][-1]) - 2 * int(d.ntails)
        self.handle = C.c_void_p()
        check(self.lib.molar_hip_membrane_plan_create(engine.ctx, C.byref(d), C.byref(self.handle)))
        engine._adopt(self)
        self._views = {}
        self._keep = {}

    def close(self):
        if getattr(self, "handle", None) and getattr(self.eng, "ctx", None):
            self.lib.molar_hip_membrane_plan_destroy(self.handle)
        self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_valid(self, valid=None):
        """valid flags for the frames to come (None: reset_valid_lipids, lib.rs:269-273)."""
        v = None if valid is None else np.ascontiguousarray(valid, np.uint8)
        check(self.lib.molar_hip_membrane_plan_set_valid(self.handle, None if v is None else v.ctypes.data))

    def set_shells(self, n_shells_patch=0, n_shells_smoothing=0):
        """n_shells_patch / n_shells_smoothing of MembraneOptions (lib.rs:53-85) for the frames to come; (0, 0) = no shells.
        No frame may be in flight."""
        check(self.lib.molar_hip_membrane_plan_set_shells(self.handle, int(n_shells_patch), int(n_shells_smoothing)))

    def begin(self, xyz, box):
        """Enqueue one frame; xyz: float32 [N,3] torch CUDA tensor (unwrapped in place) or numpy array (unwrapped in place
        as well, through a copy).  Returns the ticket."""
        pb = box if isinstance(box, PeriodicBox) else PeriodicBox.from_matrix(box)
        m9 = pb.colmajor9()
        xa, kx = _addr(xyz)
        t = C.c_int32(-1)
        check(self.lib.molar_hip_membrane_frame_begin(self.handle, xa, m9.ctypes.data, C.byref(t)))
        self._keep[t.value] = kx
        return t.value

    _PATCH_SIZED = ("patch_ids", "neib_ids", "voro_vertexes", "fitted_patch_points")

    def end(self, ticket, names=None):
        """Wait for the frame; returns its MembraneView (device addresses, sizes) - or, with `names` (per-lipid arrays and
        "order"), the pair (view, dict of numpy arrays): the arrays leave behind the frame's last kernel, one wait for both
        (molar_hip_membrane_frame_end_fetch)."""
        v = MembraneView()
        out = None
        if names is None:
            rc = self.lib.molar_hip_membrane_frame_end(self.handle, int(ticket), C.byref(v))
        else:
            if any(k in self._PATCH_SIZED for k in names):
                raise ValueError("end(names=...): per-lipid arrays and order only; fetch() brings the patch-sized arrays")
            out, o = self._arrays(names, self.K, 0)
            rc = self.lib.molar_hip_membrane_frame_end_fetch(self.handle, int(ticket), C.byref(v), C.byref(o))
        if rc == 0 or int(ticket) not in (0, 1) or v.nlipids:      # the frame is over (even if one of its stages failed)
            self._keep.pop(int(ticket), None)
        check(rc)
        self._views[int(ticket)] = v
        return v if names is None else (v, out)

    def _arrays(self, names, K, E):
        out, o = {}, MembraneOut()
        for k in names:
            dt, shp = self._SHAPES[k]
            a = np.empty(shp(K, E, E + 4 * K, self.norder), dt)         # (every element is written by the fetch)
            out[k] = a
            setattr(o, k, a.ctypes.data if a.size else None)
        return out, o

    def fetch(self, ticket, names=MEMBRANE_ARRAYS):
        """The named arrays of an ended frame as numpy arrays."""
        v = self._views[int(ticket)]
        out, o = self._arrays(names, self.K, int(v.patch_entries))
        check(self.lib.molar_hip_membrane_frame_fetch(self.handle, int(ticket), C.byref(o)))
        return out


def _search_desc_f64(kind, cutoff, xyz1, idx1=None, xyz2=None, idx2=None, box=None, pbc=0, vdw1=None, vdw2=None, ids_local=False,
                     lower=None, upper=None):
    """(molar_hip_search_desc_f64, keepalive list) of an f64 request: float64 numpy arrays or contiguous CUDA tensors (used in
    place), the box as a 3x3 matrix with the box vectors as columns."""
    def f64(a):
        if a is None:
            return None
        if hasattr(a, "data_ptr"):          # a torch tensor in HBM is used in place (float64, contiguous)
            if str(a.dtype) != "torch.float64" or not a.is_contiguous():
                raise TypeError("search_f64: device tensors must be contiguous float64")
            return a
        return np.ascontiguousarray(a, np.float64)

    def addr(a):
        return None if a is None else (a.data_ptr() if hasattr(a, "data_ptr") else a.ctypes.data)
    xyz1, xyz2, vdw1, vdw2 = f64(xyz1), f64(xyz2), f64(vdw1), f64(vdw2)
    idx1, idx2 = _sel(idx1), _sel(idx2)                            # (device index tensors: int64)
    d = SearchDescF64()
    d.kind = kind
    d.cutoff = float(cutoff) if cutoff is not None else 0.0
    keep = [xyz1, xyz2, vdw1, vdw2, idx1, idx2]
    for name, arr in (("xyz1", xyz1), ("idx1", idx1), ("xyz2", xyz2), ("idx2", idx2), ("vdw1", vdw1), ("vdw2", vdw2)):
        setattr(d, name, addr(arr))
    d.natoms1 = 0 if xyz1 is None else xyz1.reshape(-1, 3).shape[0]
    d.natoms2 = 0 if xyz2 is None else xyz2.reshape(-1, 3).shape[0]
    d.n1 = 0 if idx1 is None else idx1.shape[0]
    d.n2 = 0 if idx2 is None else idx2.shape[0]
    d.ids_local = 1 if ids_local else 0
    if box is not None:
        b9 = np.ascontiguousarray(np.asarray(box, np.float64).T).reshape(9)      # column-major: columns a, b, c
        keep.append(b9)
        d.box9 = b9.ctypes.data
        d.pbc = int(pbc)
    if lower is not None:
        lo, up = f64(lower), f64(upper)
        keep += [lo, up]
        d.lower3, d.upper3 = lo.ctypes.data, up.ctypes.data
    return d, keep


def histogram_edges_f64(hmin, hmax, nbins):
    """The f64 twin of histogram_edges: float64 [nbins + 1], edges[b] = the smallest d2 >= 0 whose f64 Histogram1D::add_one
    bin is >= b (host arithmetic of the engine, no GPU)."""
    e = np.zeros(max(int(nbins), 0) + 1, np.float64)
    check(_lib.load().molar_hip_histogram_edges_f64(float(hmin), float(hmax), int(nbins), e.ctypes.data))
    return e


def histogram_edges(hmin, hmax, nbins):
    """Exact bin edges of Histogram1D::add_one (molar_membrane/src/stats.rs:29-35) over the SQUARED distance: float32
    [nbins + 1], edges[b] = the smallest d2 >= 0 whose bin is >= b (host arithmetic of the engine, no GPU)."""
    e = np.zeros(nbins + 1, np.float32)
    check(_lib.load().molar_hip_histogram_edges(float(hmin), float(hmax), int(nbins), e.ctypes.data))
    return e


def membrane_patches_from_pairs(pairs, nlipids):
    """compute_patches' list building (molar_membrane/src/lib.rs:548-557): CSR (offsets, ids) in push order."""
    pairs = np.ascontiguousarray(pairs, np.uint32).reshape(-1, 2)
    off = np.zeros(nlipids + 1, np.uint64)
    ids = np.zeros(max(2 * len(pairs), 1), np.uint64)
    check(_lib.load().molar_hip_membrane_patches_from_pairs(pairs.ctypes.data, len(pairs), nlipids, off.ctypes.data, ids.ctypes.data))
    return off, ids[: 2 * len(pairs)]


def membrane_nth_shell_patches(valid, patch_offsets, patch_ids, nvert, neib_ids, n_shells):
    """patches_from_nth_shell (molar_membrane/src/lib.rs:562-583): new patch CSR (offsets, ids) - the n-th Voronoi
    neighbour shell for valid lipids (ids ascending), the old patch for the others.  Host arithmetic of the engine."""
    lib = _lib.load()
    v = np.ascontiguousarray(valid, np.uint8); po = np.ascontiguousarray(patch_offsets, np.uint64)
    pi = np.ascontiguousarray(patch_ids, np.uint64); nv = np.ascontiguousarray(nvert, np.uint32)
    nb = np.ascontiguousarray(neib_ids, np.uint64)
    K = len(v)
    off = np.zeros(K + 1, np.uint64)
    need = C.c_size_t(0)
    args = (K, v.ctypes.data, po.ctypes.data, pi.ctypes.data if len(pi) else None, nv.ctypes.data, nb.ctypes.data, int(n_shells))
    check(lib.molar_hip_membrane_nth_shell_patches(*args, off.ctypes.data, None, 0, C.byref(need)))
    ids = np.zeros(max(need.value, 1), np.uint64)
    check(lib.molar_hip_membrane_nth_shell_patches(*args, off.ctypes.data, ids.ctypes.data, need.value, C.byref(need)))
    return off, ids[: need.value]


def membrane_smooth_curvature(valid, patch_offsets, nvert, neib_ids, n_shells, mean_curv, gauss_curv):
    """smooth_curvature (lib.rs:584-621): returns the smoothed (mean, gaussian) curvature arrays."""
    lib = _lib.load()
    v = np.ascontiguousarray(valid, np.uint8); po = np.ascontiguousarray(patch_offsets, np.uint64)
    nv = np.ascontiguousarray(nvert, np.uint32); nb = np.ascontiguousarray(neib_ids, np.uint64)
    f64 = np.asarray(mean_curv).dtype == np.float64          # float64 curvatures: the f64 entry
    real = np.float64 if f64 else np.float32
    fn = lib.molar_hip_membrane_smooth_curvature_f64 if f64 else lib.molar_hip_membrane_smooth_curvature
    m = np.array(mean_curv, real, order="C"); g = np.array(gauss_curv, real, order="C")
    check(fn(len(v), v.ctypes.data, po.ctypes.data, nv.ctypes.data, nb.ctypes.data, int(n_shells), m.ctypes.data, g.ctypes.data))
    return m, g


def membrane_initial_normals(head_markers, tail_markers, patch_offsets, patch_ids, valid=None, normals=None):
    """Membrane::compute_initial_normals (molar_membrane/src/lib.rs:456-505); host arithmetic of the engine."""
    lib = _lib.load()
    f64 = np.asarray(head_markers).dtype == np.float64       # float64 markers: the f64 entry
    real = np.float64 if f64 else np.float32
    fn = lib.molar_hip_membrane_initial_normals_f64 if f64 else lib.molar_hip_membrane_initial_normals
    head = np.ascontiguousarray(head_markers, real); tail = np.ascontiguousarray(tail_markers, real)
    po = np.ascontiguousarray(patch_offsets, np.uint64); pi = np.ascontiguousarray(patch_ids, np.uint64)
    K = len(head)
    out = np.zeros((K, 3), real) if normals is None else np.ascontiguousarray(normals, real)
    v = None if valid is None else np.ascontiguousarray(valid, np.uint8)
    check(fn(K, head.ctypes.data, tail.ctypes.data, po.ctypes.data, pi.ctypes.data if len(pi) else None,
             None if v is None else v.ctypes.data, out.ctypes.data))
    return out


# ---------------------------------------------------------------- pymolar-style front-end

_default_engine = None


def default_engine() -> Engine:
    global _default_engine
    if _default_engine is None:
        _default_engine = Engine(0)
    return _default_engine


class State:
    """Coordinates + box of one frame (state.rs:22-28)."""

    def __init__(self, coords, box: PeriodicBox | None = None, time: float = 0.0):
        self.coords = _f32(coords)
        self.pbox = box
        self.time = time

    def __len__(self):
        return self.coords.shape[0]


class Topology:
    """Only the per-atom columns the path reads: masses and vdW radii (atom_storage.rs:272)."""

    def __init__(self, masses, vdw=None):
        self.masses = _f32(masses)
        self.vdw = _f32(vdw)


def rotation_from_axis_angle(axis, angle):
    """nalgebra Rotation3::from_axis_angle (Rodrigues), f32; `axis` is normalised like Unit::new_normalize."""
    f = np.float32
    u = np.asarray(axis, f)
    u = (u / f(np.sqrt(f(f(u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])))).astype(f)
    ux, uy, uz = u
    s, c = f(np.sin(f(angle))), f(np.cos(f(angle)))
    k = f(1) - c
    sqx, sqy, sqz = ux * ux, uy * uy, uz * uz
    return np.array([[sqx + (f(1) - sqx) * c, ux * uy * k - uz * s, ux * uz * k + uy * s],
                     [ux * uy * k + uz * s, sqy + (f(1) - sqy) * c, uy * uz * k - ux * s],
                     [ux * uz * k - uy * s, uy * uz * k + ux * s, sqz + (f(1) - sqz) * c]], dtype=f)


class Sel:
    """A bound selection: sorted, non-empty index set over (Topology, State) (sel.rs:10-31)."""

    def __init__(self, top: Topology, state: State, index=None, engine: Engine | None = None):
        n = len(state)
        if index is None:
            index = np.arange(n, dtype=np.uint64)
        index = np.unique(np.asarray(index, dtype=np.uint64))     # SVec: sorted + dedup
        if len(index) == 0:
            raise ValueError("selection is empty")                 # sel.rs:13-19
        self.top, self.state, self.index = top, state, index
        self._engine = engine

    @property
    def engine(self):
        """The GPU context is created on first use, so selections can be built without a device."""
        if self._engine is None:
            self._engine = default_engine()
        return self._engine

    def __len__(self):
        return len(self.index)

    def require_box(self) -> PeriodicBox:
        if self.state.pbox is None:
            raise MolarHipError(4, "pbc operation without periodic box")
        return self.state.pbox

    # molar_python/src/selection.rs:816-829 — com(dims) always goes through the pbc variant
    def com(self, dims=None):
        if dims is None or pbc_mask(dims) == 0:
            return self.engine.center_of_mass(self.state.coords, self.top.masses, self.index)
        return self.engine.center_of_mass_pbc(self.state.coords, self.top.masses, self.require_box(), dims, self.index)

    def cog(self, dims=None):
        if dims is None or pbc_mask(dims) == 0:
            return self.engine.center_of_geometry(self.state.coords, self.index)
        return self.engine.center_of_geometry_pbc(self.state.coords, self.require_box(), dims, self.index)

    def center_of_mass(self):
        return self.engine.center_of_mass(self.state.coords, self.top.masses, self.index)

    def center_of_geometry(self):
        return self.engine.center_of_geometry(self.state.coords, self.index)

    def gyration(self):
        return self.engine.gyration(self.state.coords, self.top.masses, self.index)

    def gyration_pbc(self):
        return self.engine.gyration(self.state.coords, self.top.masses, self.index, self.require_box())

    def inertia(self):
        m, a, _ = self.engine.inertia(self.state.coords, self.top.masses, self.index)
        return m, a

    def inertia_pbc(self):
        m, a, _ = self.engine.inertia(self.state.coords, self.top.masses, self.index, self.require_box())
        return m, a

    def min_max(self):
        return self.engine.min_max(self.state.coords, self.index)

    def sasa(self, probe=0.14, npoints=960):
        """Measure::sasa (measure.rs:427) / pymolar sel.sasa(): per-atom areas and their total, radii from the topology."""
        vdw = self.top.vdw[self.index.astype(np.int64)]
        return self.engine.sasa(self.state.coords, vdw, self.index, probe=probe, npoints=npoints)

    def sasa_vol(self, probe=0.14, npoints=960):
        """Measure::sasa_vol (measure.rs:435) / pymolar sel.sasa_vol(): areas, volumes and their totals."""
        vdw = self.top.vdw[self.index.astype(np.int64)]
        return self.engine.sasa_vol(self.state.coords, vdw, self.index, probe=probe, npoints=npoints)

    # measure.rs:100-109, 246-257, 646-649: T(cm) * inverse(axes) * T(-cm), returned as (R, t) of p -> R p + t
    def principal_transform(self):
        return self.engine.principal_transform(self.state.coords, self.top.masses, self.index)

    def principal_transform_pbc(self):
        return self.engine.principal_transform(self.state.coords, self.top.masses, self.index, self.require_box())

    # modify.rs:16-30
    def translate(self, shift):
        self.engine.translate(self.state.coords, shift, self.index)

    def rotate(self, axis, angle):
        """Rotation3::from_axis_angle about a unit axis through the origin (modify.rs:25-30); `axis` is normalised
        like Unit::new_normalize."""
        f = np.float32
        u = np.asarray(axis, f)
        u = (u / f(np.sqrt(f(f(u[0] * u[0] + u[1] * u[1]) + u[2] * u[2])))).astype(f)
        self.engine.rotate(self.state.coords, u, angle, self.index)

    def apply_transform(self, tr):
        R, t = tr
        self.engine.apply_transform(self.state.coords, R, t, self.index)

    def unwrap_simple(self, dims=PBC_FULL):
        self.engine.unwrap_simple(self.state.coords, self.require_box(), dims, self.index)

    def within(self, cutoff, inner: "Sel", pbc=None, include_inner=False):
        """`within <cutoff> [pbc xyz] [self] of <inner>` evaluated inside this selection
        (LogicalNode::Within, selection/ast.rs:589-631): atoms of `self` closer than cutoff to any atom
        of `inner`; the raw search stream is sorted + de-duplicated like SVec::from_unsorted
        (selection_expr.rs:112); `include_inner` is the `self` keyword (:627-629)."""
        mask = pbc_mask(pbc)
        eng = self.engine
        if mask == 0:
            lo, up = self.min_max()                                   # ast.rs:600-602
            lo = lo + (np.float32(-cutoff) - np.float32(1.1920929e-07))
            up = up + (np.float32(cutoff) + np.float32(1.1920929e-07))
            ids = eng.within_set(cutoff, self.state.coords, self.index, inner.state.coords, inner.index, lower=lo, upper=up)
        else:
            ids = eng.within_set(cutoff, self.state.coords, self.index, inner.state.coords, inner.index,
                                 box=self.require_box(), pbc=mask)
        if include_inner:
            ids = np.union1d(ids, inner.index)
        return ids.astype(np.uint64)

    def unwrap_connectivity(self, cutoff, dims=PBC_FULL):
        """Modify::unwrap_connectivity_dim (modify.rs:72-131): neighbour search with LOCAL ids under full
        PBC (:77-78), adjacency in pair order (SearchConnectivity, connectivity.rs:19-35), then the
        reference's stack walk that pulls every connected atom to the closest image of the atom it was
        reached from - all inside the library (molar_hip_unwrap_connectivity).  Coordinates are modified in place;
        returns the list of local-index groups the reference returns as selections."""
        return self.engine.unwrap_connectivity(self.state.coords, self.require_box(), cutoff, dims, self.index)

    def split_clusters(self, cutoff, dims=None):
        """The selection split into its connected pieces at `cutoff` (clusters()): a list of `Sel`, in the order of each
        piece's first atom - the reference's split into molecules, taken by distance instead of by bonds."""
        return [Sel(self.top, self.state, self.index[part], self._engine) for part in clusters(cutoff, self, dims).split()]


def distance_search(cutoff, data1: Sel, data2: Sel | None = None, dims=None):
    """molar_python/src/lib.rs:259-376 — same dispatch table:
    float & data2 & any dim -> double_pbc; float & data2 -> double; float & any dim -> single_pbc;
    float -> single; "vdw" needs data2 (local ids converted to global, :348-354);
    "vdw" with one selection -> NotImplementedError (:355-358)."""
    eng = data1.engine
    pbc = pbc_mask(dims)
    if isinstance(cutoff, str):
        if cutoff != "vdw":
            raise TypeError(f"Unknown cutoff type {cutoff}")
        if data2 is None:
            raise NotImplementedError("VdW distance search is not yet supported for single selection")
        v1 = data1.top.vdw[data1.index.astype(np.int64)]
        v2 = data2.top.vdw[data2.index.astype(np.int64)]
        box = data1.require_box() if pbc else None
        n = eng.search_count(SEARCH_DOUBLE_VDW, None, data1.state.coords, data1.index, data2.state.coords,
                             data2.index, box=box, pbc=pbc, vdw1=v1, vdw2=v2, ids_local=True)
        i, j, d = eng.search_fill_usize(n)
        i = data1.index[i.astype(np.int64)]
        j = data2.index[j.astype(np.int64)]
        return np.stack([i, j], 1), d
    if not isinstance(cutoff, (float, int, np.floating, np.integer)):
        raise TypeError("cutoff must be a float or 'vdw'")
    if data2 is not None:
        box = data1.require_box() if pbc else None
        n = eng.search_count(SEARCH_DOUBLE, cutoff, data1.state.coords, data1.index, data2.state.coords, data2.index,
                             box=box, pbc=pbc)
    else:
        box = data1.require_box() if pbc else None
        n = eng.search_count(SEARCH_SINGLE, cutoff, data1.state.coords, data1.index, box=box, pbc=pbc)
    i, j, d = eng.search_fill_usize(n)
    return np.stack([i, j], 1), d


def contacts(cutoff, sel1: Sel, sel2: Sel | None = None, dims=None, groups1=None, groups2=None):
    """Contact counts of what distance_search(cutoff, sel1, sel2, dims) lists, without the list (same dispatch: any
    periodic dim -> the _pbc driver, two selections -> DOUBLE).  `groups1` / `groups2`: one label per selected atom
    (e.g. the residue number); the map has max(label) + 1 groups per side.  Returns a `Contacts` whose ids are positions
    in the selections."""
    eng = sel1.engine
    pbc = pbc_mask(dims)
    box = sel1.require_box() if pbc else None
    g1 = None if groups1 is None else np.ascontiguousarray(groups1, np.uint32)
    g2 = None if groups2 is None else np.ascontiguousarray(groups2, np.uint32)
    ng1 = 0 if g1 is None else int(g1.max()) + 1
    if sel2 is not None:
        if (g1 is None) != (g2 is None):
            raise ValueError("contacts: labels are needed for both selections or for none")
        ng2 = 0 if g2 is None else int(g2.max()) + 1
        return eng.search_contacts(SEARCH_DOUBLE, cutoff, sel1.state.coords, sel1.index, sel2.state.coords, sel2.index, box=box, pbc=pbc,
                                   group1=g1, ngroups1=ng1, group2=g2, ngroups2=ng2)
    return eng.search_contacts(SEARCH_SINGLE, cutoff, sel1.state.coords, sel1.index, box=box, pbc=pbc, group1=g1, ngroups1=ng1)


def clusters(cutoff, sel: Sel, dims=None, groups=None):
    """Connected components of the graph whose edges are what distance_search(cutoff, sel, dims=dims) lists (any periodic dim ->
    the _pbc driver), without the list: aggregates, leaflets, the pieces of a selection taken by distance.  `groups`: one label
    per selected atom (e.g. the residue or molecule number) - the particles are then the max(label) + 1 groups.  Returns a
    `Clusters` whose ids are positions in the selection (or labels)."""
    eng = sel.engine
    pbc = pbc_mask(dims)
    box = sel.require_box() if pbc else None
    g = None if groups is None else np.ascontiguousarray(groups, np.uint32)
    ng = 0 if g is None or g.size == 0 else int(g.max()) + 1
    return eng.search_clusters(cutoff, sel.state.coords, sel.index, box=box, pbc=pbc, group=g, ngroups=ng)


def hbond_donors(sel_heavy: Sel, sel_h: Sel, bond_cutoff=0.12, dims=None, search=None):
    """The hydrogens of every atom of `sel_heavy` as the CSR (offsets, idx) that hbonds() takes: each atom of `sel_h` goes to its
    nearest atom of `sel_heavy` within `bond_cutoff` (ties: the one listed first), found with the two-set search; a hydrogen
    with no heavy atom in reach belongs to nobody.  `dims`: periodic dimensions (None: all three when the state has a box).
    `search(cutoff, sel1, sel2, dims)` -> (pairs of atom indices, distances) replaces distance_search (tests)."""
    if dims is None:
        dims = (True, True, True) if sel_heavy.state.pbox is not None else (False, False, False)
    pairs, dist = (search or distance_search)(bond_cutoff, sel_heavy, sel_h, dims)
    return _donors_csr(np.asarray(sel_heavy.index, np.uint64), np.asarray(pairs, np.uint64).reshape(-1, 2), np.asarray(dist))


def _donors_csr(heavy_index, pairs, dist):
    pos = {int(a): p for p, a in enumerate(heavy_index)}
    best = {}
    for (i, j), d in zip(pairs.tolist(), dist.tolist()):
        cand = (d, pos[i])
        if j not in best or cand < best[j]:
            best[j] = cand
    rows = [[] for _ in range(len(heavy_index))]
    for j in sorted(best):
        rows[best[j][1]].append(j)
    off = np.zeros(len(rows) + 1, np.uint64)
    np.cumsum([len(r) for r in rows], out=off[1:])
    return off, np.asarray([j for r in rows for j in r], np.uint64)


def hbonds(donors: Sel, acceptors: Sel, hydrogens=None, dims=None, cutoff=0.35, angle=150.0, angle_kind="dha", max_ha=0.0,
           groups1=None, groups2=None, sel_h: Sel | None = None):
    """Hydrogen bonds between two selections of one state (Engine.hbonds).  `hydrogens`: as for Engine.hbonds; None: they are
    found by hbond_donors(donors, sel_h) - `sel_h` is then the selection of the hydrogens.  `dims` as for contacts();
    `groups1` / `groups2`: one label per donor / acceptor for the map.  Returns an `HBonds`."""
    eng = donors.engine
    pbc = pbc_mask(dims)
    box = donors.require_box() if pbc else None
    if hydrogens is None:
        if sel_h is None:
            raise ValueError("hbonds: without `hydrogens` the selection of the hydrogens (sel_h) is needed")
        hydrogens = hbond_donors(donors, sel_h, dims=dims)
    if (groups1 is None) != (groups2 is None):
        raise ValueError("hbonds: labels are needed for both selections or for none")
    g1 = None if groups1 is None else np.ascontiguousarray(groups1, np.uint32)
    g2 = None if groups2 is None else np.ascontiguousarray(groups2, np.uint32)
    return eng.hbonds(donors.state.coords, donors.index, hydrogens, acceptors.index, box=box, pbc=pbc, cutoff=cutoff, angle=angle,
                      angle_kind=angle_kind, max_ha=max_ha, group1=g1, ngroups1=0 if g1 is None else int(g1.max()) + 1, group2=g2,
                      ngroups2=0 if g2 is None else int(g2.max()) + 1)


def fit_transform(sel1: Sel, sel2: Sel):
    return sel1.engine.fit_transform(sel1.state.coords, sel1.top.masses, sel2.state.coords, sel2.top.masses,
                                     sel1.index, sel2.index)


def fit_transform_at_origin(sel1: Sel, sel2: Sel):
    return sel1.engine.fit_transform(sel1.state.coords, sel1.top.masses, sel2.state.coords, sel2.top.masses,
                                     sel1.index, sel2.index, at_origin=True)


def rmsd(sel1: Sel, sel2: Sel) -> float:
    return sel1.engine.rmsd(sel1.state.coords, sel2.state.coords, sel1.index, sel2.index)


rmsd_py = rmsd


def rmsd_mw(sel1: Sel, sel2: Sel) -> float:
    return sel1.engine.rmsd_mw(sel1.state.coords, sel1.top.masses, sel2.state.coords, sel1.index, sel2.index)
