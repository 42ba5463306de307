#!/usr/bin/env python3
"""isa_same.py OLD.s NEW.s - are the kernels of two device assembly files the same instructions?

The files are the `*-hip-amdgcn-amd-amdhsa-gfx950.s` that `hipcc -save-temps` leaves for one translation unit.  Each is split
into its functions (symbols typed @function; data such as MASKS64 is not code), comments and assembler directives are
dropped and `.LBB` labels are renumbered in order of appearance, so that moving or renaming source leaves nothing to differ
in.  Prints `SAME name` or `DIFF old-length new-length name` per function; exits 1 on any DIFF or any function present on one
side only."""
import re
import sys


def kernels(path):
    out, name, body = {}, None, []
    funcs = set()
    lines = open(path).read().split("\n")
    for l in lines:
        m = re.match(r"\s*\.type\s+(\S+),@function", l)
        if m:
            funcs.add(m.group(1))
    for l in lines:
        m = re.match(r"^([\w$.]+):", l)
        if m and m.group(1) in funcs:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        if re.match(r"^\.Lfunc_end\d+:", l):
            labels = {}
            text = "\n".join(body)
            for lab in re.findall(r"\.LBB\d+_\d+", text):
                labels.setdefault(lab, f".LBB_{len(labels)}")
            out[name] = [re.sub(r"\.LBB\d+_\d+", lambda x: labels[x.group(0)], b) for b in body]
            name = None
            continue
        t = l.split(";")[0].strip()
        if t and (not t.startswith(".") or re.match(r"^\.LBB\d+_\d+:", t)):
            body.append(t)
    return out


def main():
    old, new = kernels(sys.argv[1]), kernels(sys.argv[2])
    bad = 0
    for name in sorted(set(old) | set(new)):
        if name not in old or name not in new:
            print(("ONLY-OLD " if name in old else "ONLY-NEW ") + name)
            bad += 1
        elif old[name] == new[name]:
            print("SAME " + name)
        else:
            print(f"DIFF {len(old[name])} {len(new[name])} {name}")
            bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
