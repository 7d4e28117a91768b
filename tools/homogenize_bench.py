"""Times of the parcel homogenisation (crop2seg_amd/postprocess.py, csrc/parcels.hip) on one tile of the web app's size:
1098 x 1098 pixels, K = 16 classes (15 = boundary), fields of random blobs with boundary lines between them.

    python tools/homogenize_bench.py [--size 1098] [--reps 20] [--warmup 5] [--seed 1] [--soft]

Per entry point and for the two chains (homogenize_boundaries: seeds + labelling + vote; homogenize: the vote over a given
parcel raster) the script prints one JSON line: the median and the minimum of `reps` HIP-event times in microseconds, next
to the bytes each pass has to move at least (from the shapes: what is read and written once; the parent walks of the union-
find and the atomics come on top and depend on the mask).  The Python entry points allocate their outputs and workspaces per
call; that is inside the timed window, as a caller pays it.  Where scipy imports, the host time of the same work on the same
raster follows (scipy.ndimage.label with the plus element, the size filter and a numpy bincount vote: the raster part of
what the reference does on the host behind a .cpu(); its vector part is not restated).  No number here is a pass criterion.

--soft times the soft vote (postprocess.parcel_soft_vote, on probabilities and on logits) beside the hard vote instead, on two
parcel rasters: the components of the scene above (LPIS-like: hundreds of parcels, label 0 on the lines) and ONE parcel over
the whole raster, where every wave adds to the same K sums (the contention worst case).  Both votes get a table cut to the
largest id.  `read_share_of_8TBps` is 4 * K * H * W bytes (the scores, read once) / time / 8e12.
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def scene(size, k, seed, cell=24):
    """logits f32 [1,k,size,size]: one strong class per coarse cell, closed lines of class k-1 between the cells; a third of
    the cell edges is left open, so that neighbouring cells merge into random blobs of fields."""
    rng = np.random.default_rng(seed)
    n = -(-size // cell)
    up = lambda a: np.repeat(np.repeat(a, cell, 0), cell, 1)[:size, :size]      # noqa: E731
    field = up(rng.integers(0, k - 1, size=(n, n)))
    open_top, open_left = up(rng.random((n, n)) < 0.33), up(rng.random((n, n)) < 0.33)
    ys, xs = np.mgrid[0:size, 0:size]
    on_row, on_col = ys % cell == 0, xs % cell == 0
    line = (on_row & on_col) | (on_row & ~open_top) | (on_col & ~open_left)
    top = np.where(line, k - 1, field)
    logits = rng.normal(0.0, 1.0, size=(k, size, size)).astype(np.float32)
    np.put_along_axis(logits, top[None], 6.0, 0)
    return logits[None]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=1098)
    ap.add_argument("--classes", type=int, default=16)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--seed", type=int, default=1)
    ap.add_argument("--min-size", type=int, default=13)
    ap.add_argument("--soft", action="store_true", help="time the soft vote beside the hard vote on two parcel rasters")
    args = ap.parse_args()
    import torch
    from crop2seg_amd import postprocess as PP
    if not torch.cuda.is_available():
        raise SystemExit("homogenize_bench: needs an MI355X; there is no CPU path to time")
    S, K, ms = args.size, args.classes, args.min_size
    N = S * S
    host_logits = scene(S, K, args.seed)
    logits = torch.from_numpy(host_logits).cuda()
    mask, t1, _ = PP._seeds(logits, K - 1, 0.3, True, None, True)
    labels, count = PP.label_components(mask, ms)
    ncomp = int(count[0])
    cap = N // ms + 1

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        times = []
        for _ in range(args.reps):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            b.synchronize()
            times.append(a.elapsed_time(b) * 1e3)
        return {"median_us": round(statistics.median(times), 1), "min_us": round(min(times), 1)}

    if args.soft:
        proba = torch.softmax(logits, 1)
        head = {"tile": [S, S], "classes": K, "device": torch.cuda.get_device_name(0), "score_bytes": 4 * K * N}
        print(json.dumps(head), flush=True)
        for name, lab, top in (("lpis_like", labels, max(ncomp, 1)), ("one_parcel", torch.ones_like(labels), 1)):
            rows = [("parcel_vote", lambda: PP._vote(t1, lab, K, 0.75, "zero", top)),
                    ("parcel_soft_vote", lambda: PP.parcel_soft_vote(proba, lab, 0.7, False, "zero", top)),
                    ("parcel_soft_vote_from_logits", lambda: PP.parcel_soft_vote(logits, lab, 0.7, True, "zero", top))]
            for entry, fn in rows:
                row = {"scene": name, "parcels": top, "entry": entry, **timed(fn)}
                if entry != "parcel_vote":
                    row["read_share_of_8TBps"] = round(4 * K * N / (row["median_us"] * 1e-6) / 8e12, 4)
                print(json.dumps(row), flush=True)
        assert PP.check_errors() == (0, 0) and PP.nonfinite_scores() == 0
        return

    nblk = -(-N // 256)
    rows = [
        ("parcel_seeds", lambda: PP._seeds(logits, K - 1, 0.3, True, None, True),
         {"read": 4 * K * N, "write": N + 8 * N}),
        ("label_components", lambda: PP.label_components(mask, ms),
         {"init": 8 * N, "unite": N + 4 * N, "flatten": N + 8 * N, "count": 9 * N + 4 * nblk, "scan": 8 * nblk,
          "number": 9 * N + 4 * nblk, "write": N + 8 * N + 4 * N}),
        ("parcel_vote", lambda: PP._vote(t1, labels, K, None, "zero", cap),
         {"zero": 4 * cap * K, "hist": 12 * N, "winner": 4 * cap * K + 4 * cap, "write": 12 * N + 8 * N}),
        ("parcel_vote_cap_fitted", lambda: PP._vote(t1, labels, K, None, "zero", max(ncomp, 1)),
         {"zero": 4 * ncomp * K, "hist": 12 * N, "winner": 4 * ncomp * K + 4 * ncomp, "write": 12 * N + 8 * N}),
        ("homogenize_boundaries", lambda: PP.homogenize_boundaries(logits, K - 1, 0.3, True, None, ms), None),
        ("homogenize", lambda: PP.homogenize(t1, labels, K, 0.75, "zero", cap=max(ncomp, 1)), None),
    ]
    head = {"tile": [S, S], "classes": K, "min_size": ms, "components": ncomp, "seed_share": round(float(mask.float().mean()), 4),
            "device": torch.cuda.get_device_name(0)}
    print(json.dumps(head), flush=True)
    for name, fn, passes in rows:
        row = {"entry": name, **timed(fn)}
        if passes is not None:
            row["min_bytes_per_pass"] = passes
            row["min_bytes"] = sum(passes.values())
        print(json.dumps(row), flush=True)
    assert PP.check_errors() == (0, 0)
    try:
        from scipy import ndimage
    except ImportError:
        print(json.dumps({"entry": "host_restatement", "note": "scipy does not import: not measured"}), flush=True)
        return
    hm, ht1 = mask[0].cpu().numpy(), t1[0].cpu().numpy()
    plus = np.array([[0, 1, 0], [1, 1, 1], [0, 1, 0]])
    times = []
    for _ in range(3):
        t0 = time.perf_counter()
        lab, n = ndimage.label(hm, plus)
        sizes = np.bincount(lab.reshape(-1), minlength=n + 1)
        keep = sizes >= ms
        keep[0] = False
        renum = np.cumsum(keep) * keep
        lab = renum[lab]
        hist = np.bincount(lab.reshape(-1) * K + ht1.reshape(-1), minlength=(int(keep.sum()) + 1) * K).reshape(-1, K)
        hist[:, 0] = 0
        winner = hist.argmax(1)
        winner[0] = 0
        out = winner[lab]
        times.append((time.perf_counter() - t0) * 1e6)
    same = bool(np.array_equal(out, PP.homogenize_boundaries(logits, K - 1, 0.3, True, None, ms)[0].cpu().numpy()))
    print(json.dumps({"entry": "host_restatement (scipy label + numpy bincount vote, after the .cpu())",
                      "median_us": round(statistics.median(times), 1), "min_us": round(min(times), 1),
                      "equals_device_result": same}), flush=True)


if __name__ == "__main__":
    main()
