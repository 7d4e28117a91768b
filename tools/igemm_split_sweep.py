#!/usr/bin/env python
"""Tile-split sweep of c2s_conv_igemm over the launches of a step.

    python tools/igemm_split_sweep.py RECORD.json [OUT.txt]

RECORD.json is what `tools/igemm_split_launches.py record` wrote.  Every distinct c2s_conv_igemm descriptor is launched
through the C ABI with C2S_IGEMM_SPLIT = 1, 2, 4: 5 warm-up launches, then 3 windows of 40 launches back to back between
two HIP events; the figure is the best window's microseconds per launch.  Operands are random numbers (the timing does
not depend on them); the descriptor is rebuilt from the record's fields with plain output placement.  The last column is
what the rule (c2s_conv_igemm_split) picks.  The launches of c2s_conv_xpair, which has no split, are left out.
"""
import ctypes as C
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from crop2seg_amd import _lib                                   # noqa: E402
from igemm_split_launches import FIELDS, geometry                # noqa: E402


def desc_of(r):
    K = r["KH"]
    pad = {1: 0, 2: 0, 3: 1, 4: 1, 6: 2}[K]
    return _lib.ConvDesc(r["N"], r["C0"], r["C1"], r["Hin"], r["Win"], r["Cout"], r["CoutP"], r["Hout"], r["Wout"], r["Hout"],
                         r["Wout"], K, K, r["S"], pad, pad, _lib.PAD_ZEROS, 1, 1, 0, 0, r["accumulate"], r["reflect_adjoint"])


def time_launch(L, r, d, bufs):
    src0, src1, wpk, out = bufs
    call = lambda: L.c2s_conv_igemm(C.byref(d), src0.data_ptr(), src1.data_ptr() if r["C1"] else None, wpk.data_ptr(), None,
                                    out.data_ptr(), None, None)
    for _ in range(5):
        assert call() == 0, L.c2s_last_error()
    best = 1e30
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(40):
            call()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1e3 / 40)
    return best


def main():
    rec = json.load(open(sys.argv[1]))
    out = open(sys.argv[2], "w") if len(sys.argv) > 2 else None
    L = _lib.lib()
    L.c2s_init(-1)
    torch.zeros(1, device="cuda")
    seen, lines = set(), []
    lines.append("# entry(K,S) N Cin->Cout plane acc radj | wgs(1) ksteps | us at split 1 / 2 / 4 | rule")
    # besides the step's launches: 1x1 layers with few channels at 64 x 64, N = 4 (the shortest K loops the kernel has)
    extra = [dict(N=4, C0=c, C1=0, Hin=64, Win=64, Cout=32, CoutP=32, Hout=64, Wout=64, KH=1, S=1, accumulate=0,
                  reflect_adjoint=0, entry="igemm") for c in (16, 32, 48)]
    for r in rec["launches"][:len(rec["launches"]) // (rec["steps"] + rec["warmup"])] + extra:
        key = tuple(r[k] for k in FIELDS) + (r["entry"],)
        if key in seen:
            continue
        seen.add(key)
        if r["entry"] != "igemm":           # c2s_conv_xpair has no split
            continue
        env, query = "C2S_IGEMM_SPLIT", L.c2s_conv_igemm_split
        d = desc_of(r)
        Cin = r["C0"] + r["C1"]
        taps = r["KH"] ** 2
        bufs = (torch.randn(r["N"] * r["C0"] * r["Hin"] * r["Win"], device="cuda"),
                torch.randn(max(r["N"] * r["C1"] * r["Hin"] * r["Win"], 1), device="cuda"),
                torch.randn(taps * Cin * r["CoutP"], device="cuda"),
                torch.zeros(r["N"] * r["Cout"] * d.OutH * d.OutW, device="cuda"))
        us = []
        for sp in (1, 2, 4):
            os.environ[env] = str(sp)
            us.append(time_launch(L, r, d, bufs))
        os.environ.pop(env)
        wgs, ksteps = geometry(r)
        lines.append(f"{r['entry']}({r['KH']},{r['S']}) N={r['N']:<3} {Cin:>3}->{r['Cout']:<3} {r['Hout']:>3}x{r['Wout']:<3} "
                     f"acc={r['accumulate']} radj={r['reflect_adjoint']} | {wgs[0]:>5} {ksteps:>5} | "
                     f"{us[0]:6.1f} {us[1]:6.1f} {us[2]:6.1f} | {query(C.byref(d), 0)}")
        print(lines[-1], flush=True)
    if out:
        out.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
