"""Bits of the four criteria of csrc/loss.hip from two builds of the library, side by side.

    C2S_LIB=/path/to/libc2s_hip.so python tools/loss_ab.py dump OUT.npz
    python tools/loss_ab.py compare A.npz B.npz
    python tools/loss_ab.py time A.so B.so

dump     runs cross entropy, focal CE, smooth CE and recall CE on every row of the tables of tests/test_tail_reference_gpu.py
         (CE_ROWS and the all-ignored row, FOCAL_ROWS, SMOOTH_ROWS) and tests/test_recall_reference_gpu.py (ROWS), built by
         the tables' own seeded builders and called as the tests call them, and on the two inputs tools/recall_bench.py times
         (B4 K15 128 x 128, B8 K15 256 x 256).  Saved: the loss, glogits, pixel_loss, recall's weights and counts, and the
         documented words of each workspace (tot[] and the bad-target counts, recall's nll and w[K]) -- not the block
         partials, which are uninitialised past `blocks`.  The library is the one C2S_LIB names (crop2seg_amd/_lib.py), one
         process per library.
compare  demands the same keys, shapes, types and bytes (NaN payloads included); prints every difference and exits 1 on any.
time     loads both libraries into ONE process and times the four entry points with gradient on the same buffers at the two
         sizes of tools/recall_bench.py, 7 alternating windows of 200 calls each.  Between processes the loss calls have two
         timing states several microseconds apart, whichever library is loaded (profiles/loss_shared_ab.txt), so a difference of
         a per cent between two builds shows only inside one process.
"""
import ctypes
import json
import os
import statistics
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tools")]


def dump(path):
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("loss_ab: needs an MI355X (no CPU fallback)")
    import recall_bench
    import test_recall_reference_gpu as TR
    import test_tail_reference_gpu as TT
    from crop2seg_amd import _lib
    from crop2seg_amd import engine as E
    from crop2seg_amd.learning import losses
    out = {}

    def put(name, **tensors):
        for k, v in tensors.items():
            if v is not None:
                out[f"{name}/{k}"] = v.detach().cpu().numpy()

    def cuda(t):
        return None if t is None else t.cuda()

    def recall(name, z, t, ignore):
        B, K, n = z.shape[0], z.shape[1], z.shape[0] * z[0, 0].numel()
        ws = E.Workspace(z.device)
        loss, gl, weights, counts = losses.recall_ce(z, t, ignore, True, ws)
        size = _lib.lib().c2s_recall_ce_workspace_floats(B, n // B)
        buf = ws.bufs["recall"]
        w0 = size - 2 - losses.RECALL_MAX_CLASSES
        put(name, loss=loss, glogits=gl, weights=weights, counts=counts, nll=buf[:n], ws_w=buf[w0:w0 + K], tot=buf[size - 2:size])

    for row in TT.CE_ROWS + [TT.CE_ALL_IGNORED]:
        z, t, kw = TT.ce_args(row)
        cw = torch.ones(row["K"]) if kw["class_w"] is None else kw["class_w"]
        ws = E.Workspace(torch.device("cuda"))
        loss, gl = E.cross_entropy(z.cuda(), t.cuda(), cw.cuda(), ws, True, kw["label_smoothing"], kw["ignore_index"])
        put(row["name"], loss=loss, glogits=gl, tot=ws.bufs["ce"][-3:])
    for row in TT.FOCAL_ROWS:
        z, t, kw = TT.focal_args(row)
        ws = E.Workspace(torch.device("cuda"))
        loss, gl = losses.focal_ce(z.cuda(), t.cuda(), kw["gamma"], kw["ignore_index"], True, ws, cuda(kw["prior"]),
                                   cuda(kw["class_w"]), kw["size_average"])
        put(row["name"], loss=loss, glogits=gl, tot=ws.bufs["focal"][-4:-1])
    for row in TT.SMOOTH_ROWS:
        z, t, kw = TT.smooth_args(row)
        ws = E.Workspace(torch.device("cuda"))
        want_pl = kw["reduction"] == "none" or row.get("pl", False)
        pl = torch.full(t.shape, float("nan"), device="cuda") if want_pl else None
        loss, gl, counters = losses.smooth_ce(z.cuda(), t.cuda(), kw["label_smoothing"], cuda(kw["class_w"]), cuda(kw["bg"]),
                                              kw["bg_index"], row.get("want_grad", True), ws, None, kw["reduction"], pl)
        put(row["name"], loss=loss, glogits=gl, pixel_loss=pl, tot=counters)
    for row in TR.ROWS:
        z, t = TR.make_inputs(row)
        recall(row["name"], z.cuda(), t.cuda(), TR.ignore_index(row))
    for B, hw in recall_bench.SHAPES:
        z, y, cw = recall_bench.loss_inputs(B, hw)
        name = f"timed_b{B}_hw{hw}"
        for ls in (0.0, 0.1):
            ws = E.Workspace(z.device)
            loss, gl = E.cross_entropy(z, y, cw, ws, True, ls)
            put(f"{name}/ce_ls{ls}", loss=loss, glogits=gl, tot=ws.bufs["ce"][-3:])
        ws = E.Workspace(z.device)
        loss, gl = losses.focal_ce(z, y, 2.0, 255, True, ws)
        put(f"{name}/focal", loss=loss, glogits=gl, tot=ws.bufs["focal"][-4:-1])
        loss, gl, counters = losses.smooth_ce(z, y, 0.1, want_grad=True, ws=ws)
        put(f"{name}/smooth", loss=loss, glogits=gl, tot=counters)
        recall(f"{name}/recall", z, y, 255)
    torch.cuda.synchronize()
    np.savez(path, **out)
    print(f"loss_ab dump: {len(out)} arrays, {sum(v.nbytes for v in out.values())} bytes, library {_lib.LIB_PATH}")


def compare(pa, pb):
    a, b = np.load(pa), np.load(pb)
    bad = [f"only in one file: {k}" for k in sorted(set(a.files) ^ set(b.files))]
    nbytes = 0
    for k in sorted(set(a.files) & set(b.files)):
        x, y = a[k], b[k]
        if x.shape != y.shape or x.dtype != y.dtype:
            bad.append(f"{k}: {x.dtype}{x.shape} against {y.dtype}{y.shape}")
            continue
        nbytes += x.nbytes
        diff = np.frombuffer(x.tobytes(), np.uint8) != np.frombuffer(y.tobytes(), np.uint8)
        if diff.any():
            bad.append(f"{k}: {int(diff.sum())} of {x.nbytes} bytes differ")
    for line in bad:
        print(line)
    print(f"loss_ab compare: {len(a.files)} / {len(b.files)} arrays, {nbytes} bytes compared, {len(bad)} differences")
    return 1 if bad or not a.files else 0


def time_libraries(path_a, path_b):
    import torch
    import recall_bench
    from crop2seg_amd import _lib

    def load(path):
        h = ctypes.CDLL(path)
        for name, (res, args) in _lib.SIGNATURES.items():
            fn = getattr(h, name)
            fn.restype, fn.argtypes = res, args
        assert h.c2s_init(torch.cuda.current_device()) == 0, path
        return h

    def calls(h, z, y, cw, loss, gl, ws, weights, counts):
        B, K, H, W = z.shape
        HW, st, n = H * W, torch.cuda.current_stream().cuda_stream, ws.numel()
        p = torch.Tensor.data_ptr
        return {
            "cross_entropy": lambda: h.c2s_cross_entropy(p(z), p(y), p(cw), p(loss), p(gl), B, K, HW, 0.0, -100, p(ws), n, st),
            "recall_ce": lambda: h.c2s_recall_ce(p(z), p(y), p(loss), p(gl), p(weights), p(counts), B, K, HW, 255, 0, p(ws), n, st),
            "focal_ce": lambda: h.c2s_focal_ce_ex(p(z), p(y), None, p(loss), p(gl), B, K, HW, 2.0, 255, 1, 0, p(ws), n, st),
            "smooth_ce": lambda: h.c2s_smooth_ce_ex(p(z), p(y), None, None, p(loss), p(gl), None, B, K, H, W, 0.1, 0, 0, 0, p(ws), n,
                                                    st),
        }

    a, b = load(path_a), load(path_b)
    for B, hw in recall_bench.SHAPES:
        z, y, cw = recall_bench.loss_inputs(B, hw)
        loss, gl = torch.empty(1, device="cuda"), torch.empty_like(z)
        ws = torch.empty(b.c2s_recall_ce_workspace_floats(B, hw * hw), device="cuda")      # the largest of the four
        weights, counts = torch.empty(z.shape[1], device="cuda"), torch.empty(2, z.shape[1], device="cuda", dtype=torch.int64)
        ca, cb = (calls(h, z, y, cw, loss, gl, ws, weights, counts) for h in (a, b))
        for name in ca:
            assert ca[name]() == 0 and cb[name]() == 0, name
            ta, tb = recall_bench.pairs([ca[name], cb[name]], 200, 7, 3)
            print(json.dumps({"B": B, "hw": hw, "criterion": name, "a_us": recall_bench.stats(ta, 1e3, 2),
                              "b_us": recall_bench.stats(tb, 1e3, 2),
                              "b_over_a": round(statistics.median(tb) / statistics.median(ta), 4)}), flush=True)


def main():
    if len(sys.argv) == 3 and sys.argv[1] == "dump":
        dump(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "time":
        time_libraries(sys.argv[2], sys.argv[3])
    elif len(sys.argv) == 4 and sys.argv[1] == "compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    else:
        raise SystemExit(__doc__)


if __name__ == "__main__":
    main()
