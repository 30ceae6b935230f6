#!/usr/bin/env python3
"""Static vector-instruction counts of k_s2m_iterate<1,false,false> between landmarks of its gfx950 assembly.

  hipcc --offload-arch=gfx950 -O3 -ffp-contract=off -std=c++17 --cuda-device-only -S -o k.s lio-slam_amd/csrc/lio_kernels.hip
  python tools/count_valu.py k.s

Segments (straight-line code every wave executes once per iteration, in program order):
  head+setup   entry .. first v_min_f64/v_max_f64          block descriptor, point loads, transform, cells, search bound, rows
  loop         first .. last v_min_f64/v_max_f64           candidate loop and the top-5 network (all unrolled copies)
  association  last v_min_f64/v_max_f64 .. ds_write_b128   gate, winner gathers, plane fit, plane test, weight, Jacobian row
  tail         ds_write_b128 .. s_endpgm                   row to LDS, fp64 sums, arrive, the Gauss-Newton step of the last workgroup
The counts are static: what the compiler emitted, not what a wave issues (branches skip parts of the association).
"""
import collections
import re
import sys

KERNEL = "_Z13k_s2m_iterateILi1ELb0ELb0EEv13LioIterParams"


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


def main():
    ins = body(sys.argv[1], sys.argv[2] if len(sys.argv) > 2 else KERNEL)
    mm = [i for i, m in enumerate(ins) if m in ("v_min_f64", "v_max_f64", "v_min_f64_e32", "v_max_f64_e32", "v_min_f64_e64", "v_max_f64_e64")]
    w = [i for i, m in enumerate(ins) if m.startswith("ds_write_b128")]
    first, last, row = mm[0], mm[-1], [i for i in w if i > mm[-1]][0]
    segs = [("head+setup", 0, first), ("loop", first, last + 1), ("association", last + 1, row), ("tail", row, len(ins))]
    for name, a, b in segs:
        v = [m for m in ins[a:b] if m.startswith("v_")]
        c = collections.Counter(re.sub(r"_e(32|64)$|_dpp$|_sdwa$", "", m) for m in v)
        pick = {k: sum(n for m, n in c.items() if m.startswith(k)) for k in
                ("v_cndmask", "v_mov", "v_cmp", "v_div_scale", "v_rcp_f32", "v_div_fmas", "v_div_fixup", "v_sqrt", "v_fma_f32", "v_fma_f64")}
        br = sum(1 for m in ins[a:b] if m.startswith(("s_cbranch", "s_branch")))
        print(f"{name:12s} VALU {len(v):5d}  all {b - a:5d}  branches {br:3d}  " + " ".join(f"{k[2:]}={n}" for k, n in pick.items() if n))


if __name__ == "__main__":
    main()
