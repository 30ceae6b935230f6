#!/usr/bin/env python3
"""Static instruction counts of one k_s2m_iterate instantiation between landmarks of its gfx950 assembly.

  hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -std=c++17 --cuda-device-only -S -o k.s lio-slam_amd/csrc/lio_kernels.hip
  python tools/count_valu.py k.s                 the plain instantiation (PPT 1, global candidates, the batch path of one device)
  python tools/count_valu.py k.s general         the general one-point instantiation
  python tools/count_valu.py k.s old             its name before the PLAIN template parameter (assembly of older trees)
  python tools/count_valu.py k.s <mangled name>  any other kernel of the file

Segments (straight-line code every wave executes once per iteration, in program order):
  head+setup   entry .. first v_min_f64/v_max_f64          block descriptor, point loads, transform, cells, search bound, rows
  loop         first .. last v_min_f64/v_max_f64           candidate loop and the top-5 network (all unrolled copies)
  association  last v_min_f64/v_max_f64 .. ds_write_b128   gate, winner gathers, plane fit, plane test, weight, Jacobian row
  row..arrive  ds_write_b128 .. the arrival atomic         row to LDS, fp64 sums, partial sums, arrival on the scan's counter
  tail         the arrival atomic .. s_endpgm              the Gauss-Newton step of the scan's last workgroup
The counts are static: what the compiler emitted, not what a wave issues (branches skip parts of the association).
`scratch`, `readlane`, `writelane` count spill traffic: scratch_* accesses and the lane moves of SGPR spills.  The last line
sums them over everything before the arrival atomic, the part every wave of every workgroup runs.
"""
import collections
import re
import sys

KERNELS = {
    "plain": "_Z13k_s2m_iterateILi1ELb0ELb0ELb1EEv13LioIterParams",
    "general": "_Z13k_s2m_iterateILi1ELb0ELb0ELb0EEv13LioIterParams",
    "old": "_Z13k_s2m_iterateILi1ELb0ELb0EEv13LioIterParams",
}
MINMAX = ("v_min_f64", "v_max_f64", "v_min_f64_e32", "v_max_f64_e32", "v_min_f64_e64", "v_max_f64_e64")


def body(path, name):
    out, on = [], False
    for line in open(path):
        if line.startswith(name + ":"):
            on = True
            continue
        if on:
            if line.startswith(".Lfunc_end"):
                break
            t = line.strip()
            if t and not t.startswith((";", ".", "//")) and not t.endswith(":"):
                out.append(t.split()[0])
    return out


def spill_counts(ins):
    return {"scratch": sum(1 for m in ins if m.startswith("scratch_")),
            "readlane": sum(1 for m in ins if m.startswith("v_readlane_b32")),
            "writelane": sum(1 for m in ins if m.startswith("v_writelane_b32")),
            "s_nop": sum(1 for m in ins if m == "s_nop")}


def main():
    which = sys.argv[2] if len(sys.argv) > 2 else "plain"
    name = KERNELS.get(which, which)
    ins = body(sys.argv[1], name)
    if not ins:
        sys.exit(f"{name} is not in {sys.argv[1]}")
    print(f"# {name}: {len(ins)} instructions")
    mm = [i for i, m in enumerate(ins) if m in MINMAX]
    w = [i for i, m in enumerate(ins) if m.startswith("ds_write_b128")]
    first, last, row = mm[0], mm[-1], [i for i in w if i > mm[-1]][0]
    # the arrival: the first global atomic after the row store (the partial sums before it are plain sc1 stores)
    arrive = [i for i, m in enumerate(ins) if i > row and m.startswith(("global_atomic", "flat_atomic"))][0]
    segs = [("head+setup", 0, first), ("loop", first, last + 1), ("association", last + 1, row), ("row..arrive", row, arrive),
            ("tail", arrive, len(ins))]
    for seg, a, b in segs:
        v = [m for m in ins[a:b] if m.startswith("v_")]
        c = collections.Counter(re.sub(r"_e(32|64)$|_dpp$|_sdwa$", "", m) for m in v)
        pick = {k: sum(n for m, n in c.items() if m.startswith(k)) for k in
                ("v_cndmask", "v_mov", "v_cmp", "v_div_scale", "v_rcp_f32", "v_div_fmas", "v_div_fixup", "v_sqrt", "v_fma_f32", "v_fma_f64")}
        br = sum(1 for m in ins[a:b] if m.startswith(("s_cbranch", "s_branch")))
        sp = spill_counts(ins[a:b])
        print(f"{seg:12s} VALU {len(v):5d}  all {b - a:5d}  branches {br:3d}  " + " ".join(f"{k}={n}" for k, n in sp.items()) + "  |  " +
              " ".join(f"{k[2:]}={n}" for k, n in pick.items() if n))
    sp = spill_counts(ins[:arrive])
    print("before the arrival atomic: " + " ".join(f"{k}={n}" for k, n in sp.items() if k != "s_nop"))


if __name__ == "__main__":
    main()
