#!/usr/bin/env python
"""The implicit-GEMM and transposed-row launches of one train step, launch by launch (profiles/igemm_split_launches.txt).

record:  rocprofv3 --kernel-trace --stats -d TRACE --output-format csv -- \
             python tools/igemm_split_launches.py record RECORD.json [bench.py arguments]
         runs bench.py in this process with engine._run_conv wrapped: every launch of c2s_conv_igemm / c2s_conv_xpair is written
         to RECORD.json in launch order with the layer (weight name), the operation, its descriptor and, where the library
         has the query (c2s_conv_igemm_split), the tile split it reports for it.  Run it with
         C2S_WGRAD_STREAM=0: the kernels of a single-stream trace are in launch order.
table:   python tools/igemm_split_launches.py table OUT.txt TRACE RECORD.json [TRACE2 RECORD2.json]
         joins the conv_igemm_kernel / conv_xpair_kernel rows of the kernel trace with the record (same order, same count)
         and prints one line per launch of a step: durations are the mean and the minimum over the timed steps (the
         warm-up steps are left out).  With a second pair the table carries both ("before" / "after").
"""
import csv
import glob
import json
import os
import runpy
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CK = {1: 16, 2: 8, 3: 4, 4: 2, 6: 2}        # channels per chunk of conv_igemm.hip; conv_xpair.hip: 4
FIELDS = ("N", "C0", "C1", "Hin", "Win", "Cout", "CoutP", "Hout", "Wout", "KH", "S", "accumulate", "reflect_adjoint")


def record(out, bench_args):
    sys.path.insert(0, ROOT)
    from crop2seg_amd import engine as E
    import ctypes as C
    log = []
    inner = E._run_conv

    def run_conv(ctx, plan, wname, *rest):
        entry = E.CONV_FAMILIES[plan.family][0]
        if entry in ("c2s_conv_igemm", "c2s_conv_xpair"):
            query = getattr(E.lib(), entry + "_split", None)
            for launch in plan.launches:
                d, key = launch[0], launch[1]
                row = {k: int(getattr(d, k)) for k in FIELDS}
                row.update(layer=wname, op=str(key[0]), entry=entry[9:],
                           split=int(query(C.byref(d), 0)) if query is not None else 1)
                log.append(row)
        return inner(ctx, plan, wname, *rest)

    E._run_conv = run_conv
    sys.argv = [os.path.join(ROOT, "bench.py")] + bench_args
    try:
        runpy.run_path(sys.argv[0], run_name="__main__")
    finally:
        steps = 20 if "--steps" not in bench_args else int(bench_args[bench_args.index("--steps") + 1])
        warm = 5 if "--warmup" not in bench_args else int(bench_args[bench_args.index("--warmup") + 1])
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        json.dump({"steps": steps, "warmup": warm, "launches": log}, open(out, "w"))


def geometry(r):
    """Workgroups of the launch at split 1 / 2 / 4 (c2s_conv_xpair has no split: its one grid three times) and the MFMA
    k-steps of one wave's K loop (host arithmetic of the two entry points)."""
    l2 = 5
    while l2 > 2 and (1 << l2) > r["Wout"]:
        l2 -= 1
    FC, FR = 1 << l2, 32 >> l2
    igemm = r["entry"] == "igemm"
    cb = r["CoutP"] // 32
    wgs = [-(-r["Wout"] // FC) * -(-r["Hout"] // ((8 // sp if igemm else 4) * FR)) * r["N"] * cb for sp in (1, 2, 4)]
    if r["entry"] == "igemm":
        ck = CK[r["KH"]]
        ksteps = (-(-r["C0"] // ck) + -(-r["C1"] // ck)) * r["KH"] * r["KH"] * (ck // 2)
    else:
        ksteps = -(-r["C0"] // 4) * 4 * 2
    return wgs, ksteps


def join(trace, rec):
    f = glob.glob(trace + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = [r for r in csv.DictReader(open(f)) if "conv_igemm_kernel" in r["Kernel_Name"] or "conv_xpair_kernel" in r["Kernel_Name"]]
    rows.sort(key=lambda r: int(r["Start_Timestamp"]))
    rec = json.load(open(rec))
    log, nsteps = rec["launches"], rec["steps"] + rec["warmup"]
    assert len(rows) == len(log), f"{len(rows)} kernels in the trace, {len(log)} launches recorded"
    assert len(log) % nsteps == 0
    per = len(log) // nsteps
    out = []
    for i in range(per):
        r = dict(log[i])
        assert all(log[i + s * per] == log[i] for s in range(nsteps)), "the steps do not repeat the same launches"
        ks = [rows[i + s * per] for s in range(rec["warmup"], nsteps)]
        us = [(int(k["End_Timestamp"]) - int(k["Start_Timestamp"])) / 1e3 for k in ks]
        name = ks[0]["Kernel_Name"]
        r["kernel"] = name[name.index("conv_"):].split("(")[0].replace("void ", "").replace(" ", "")
        r["mean_us"], r["min_us"] = sum(us) / len(us), min(us)
        if "Grid_Size_X" in ks[0]:
            g = [int(ks[0][f"Grid_Size_{a}"]) // max(int(ks[0][f"Workgroup_Size_{a}"]), 1) for a in "XYZ"]
            r["grid_wgs"] = g[0] * g[1] * g[2]
        out.append(r)
    return out


def table(out, pairs, cus=256):
    sets = [join(t, r) for t, r in pairs]
    names = ["before", "after"][:len(sets)]
    lines = ["# conv_igemm_kernel / conv_xpair_kernel launches of one U-TAE step (B=4, T=32, 128x128), single-stream kernel trace",
             "# (C2S_WGRAD_STREAM=0 rocprofv3 --kernel-trace --stats -- bench.py --steps 5 --warmup 2), in launch order; durations in us,",
             "# mean (min) over the 5 timed steps.  wgs(1) = workgroups of the launch without a split; target = fewer than 2 per CU",
             f"# ({cus} CUs); ksteps = MFMA k-steps of a wave's K loop; split = what the library's rule picks (1: no query).",
             "#",
             "# idx layer op kernel(K,S) N Cin->Cout plane_out acc radj | wgs(1) wgs(2) wgs(4) ksteps target | "
             + " | ".join(f"{n}: split grid mean (min)" for n in names)]
    tot = [[0.0, 0.0] for _ in sets]
    for i, r in enumerate(sets[0]):
        wgs, ksteps = geometry(r)
        target = wgs[0] < 2 * cus
        cols = []
        for si, s in enumerate(sets):
            q = s[i]
            assert all(q[k] == r[k] for k in FIELDS + ("layer", "op", "entry")), "the two records list different launches"
            cols.append(f"{q['split']} {q.get('grid_wgs', '-'):>5} {q['mean_us']:7.1f} ({q['min_us']:.1f})")
            tot[si][0 if target else 1] += q["mean_us"]
        lines.append(f"{i:3d} {r['layer']:<34} {r['op']:<5} {r['entry']}({r['KH']},{r['S']}) N={r['N']:<3} "
                     f"{r['C0'] + r['C1']:>3}->{r['Cout']:<3} {r['Hout']:>3}x{r['Wout']:<3} acc={r['accumulate']} radj={r['reflect_adjoint']} | "
                     f"{wgs[0]:>5} {wgs[1]:>5} {wgs[2]:>5} {ksteps:>5} {'yes' if target else 'no ':<3} | " + " | ".join(cols))
    for n, t in zip(names, tot):
        lines.append(f"# {n}: targets (wgs(1) < {2 * cus}) {t[0] / 1e3:.3f} ms per step, the other launches {t[1] / 1e3:.3f} ms")
    open(out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines[-len(sets):]))


if __name__ == "__main__":
    if sys.argv[1] == "record":
        record(sys.argv[2], sys.argv[3:])
    else:
        a = sys.argv[3:]
        table(sys.argv[2], [(a[i], a[i + 1]) for i in range(0, len(a), 2)])
