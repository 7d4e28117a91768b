"""Golden fixtures of RecallCrossEntropy from the IMPORTED reference module (src/learning/recall_loss.py), run on the CPU.
Needs the reference sources on PYTHONPATH:

    PYTHONPATH=<reference checkout>:. python tools/make_golden_recall.py

Writes tests/golden/tail_recall_*.npz (the tail_ prefix keeps them out of conftest.golden_names()): float64 logits, target,
ignore_index, and the loss and the autograd gradient of the reference's criterion.  A few hundred pixels each.

The cases are chosen so that the reference runs and means what csrc/loss.hip computes (the
RecallCrossEntropy deviations): at least two distinct labels, at least two of them misclassified; ignored pixels only with
ignore_index = -1 and then class 1 present with a false negative.  Each condition is asserted here, and so is the agreement
with tests/recall_ref.py.
"""
import os
import sys

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from src.learning.recall_loss import RecallCrossEntropy  # noqa: E402  (reference)

import recall_ref as RR  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden")

#        name            K   B  H   W   seed  ignore  ignored pixels  integer logits
CASES = [("k2",          2,  2, 12, 12, 11,   255,    False,          False),
         ("k15",         15, 2, 12, 12, 12,   255,    False,          False),
         ("k20",         20, 3, 9,  11, 13,   255,    False,          False),
         ("k15_ties",    15, 2, 12, 12, 14,   255,    False,          True),
         ("k15_ign",     15, 2, 12, 12, 15,   -1,     True,           False),
         ("k20_ign",     20, 2, 10, 13, 16,   -1,     True,           False),
         ("k2_ign_ties", 2,  2, 12, 12, 17,   -1,     True,           True)]


def make_case(K, B, H, W, seed, ignore, ignored, ties):
    gen = torch.Generator().manual_seed(seed)
    t = torch.randint(0, K, (B, H, W), generator=gen)
    z = torch.randn(B, K, H, W, generator=gen, dtype=torch.float64) * 2
    z += 2.5 * torch.nn.functional.one_hot(t, K).permute(0, 3, 1, 2)        # recall well between 0 and 1
    if ties:
        z = torch.round(z)
    if ignored:
        t[torch.rand(B, H, W, generator=gen) < 0.2] = ignore
    return z, t


def main():
    for name, K, B, H, W, seed, ignore, ignored, ties in CASES:
        z, t = make_case(K, B, H, W, seed, ignore, ignored, ties)
        pred, valid, gt, fn, bad, w = RR.recall_counts(z, t, ignore)
        assert bad == 0 and (gt > 0).sum() >= 2 and (fn > 0).sum() >= 2, name
        assert bool((t == ignore).any()) == ignored
        if ignored:
            assert ignore == -1 and fn[1] >= 1, name
        if ties:
            key = z.permute(0, 2, 3, 1).reshape(-1, K)
            assert int((key == key.max(1, keepdim=True).values).sum(1).gt(1).sum()) > 0, name
        zz = z.clone().requires_grad_(True)
        loss = RecallCrossEntropy(n_classes=K, ignore_index=ignore)(zz, t)
        loss.backward()
        ref, _ = RR.recall_ref(z, t, ignore, bounds=False)
        value = float(loss.detach())
        assert abs(value - float(ref["loss"])) <= 1e-6 * abs(value), (name, value, float(ref["loss"]))
        np.savez_compressed(os.path.join(OUT, f"tail_recall_{name}.npz"), logits=z.numpy(), target=t.numpy(),
                            ignore_index=np.int64(ignore), loss=np.float64(value), glogits=zz.grad.numpy())
        print(f"tail_recall_{name}: {B * H * W} pixels, loss {value:.6f}, fn {fn.tolist()}, gt {gt.tolist()}")


if __name__ == "__main__":
    main()
