"""Golden fixtures of the stride-2 down / up convolution geometries (str_conv_k, str_conv_s, str_conv_p) = (2, 2, 0) and
(6, 2, 2), from the imported reference models (oracle/make_golden.run_case).  Needs the reference sources on PYTHONPATH:

    PYTHONPATH=<reference checkout>:. python tools/make_golden_geometry.py

Writes tests/golden/{utae,timeunet,wtae}_*_k{2,6}_tame.npz; conftest.golden_names() picks them up.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

from oracle.make_golden import run_case  # noqa: E402

K2 = dict(str_conv_k=2, str_conv_s=2, str_conv_p=0)
K6 = dict(str_conv_k=6, str_conv_s=2, str_conv_p=2)


def main():
    torch.set_num_threads(8)
    run_case("utae_train_k2_tame", "utae", "tame", 201, 211, 2, 5, 16, [5, 3], "train", ctor=dict(K2))
    run_case("utae_eval_k6_tame", "utae", "tame", 202, 212, 2, 5, 16, [5, 4], "eval", ctor=dict(K6))
    run_case("utae_train_drop_k6_tame", "utae", "tame", 223, 233, 2, 5, 16, [5, 4], "train", dropout=80, ctor=dict(K6))
    run_case("timeunet_train_k6_tame", "timeunet", "tame", 204, 214, 1, 4, 16, None, "train", ctor=dict(K6))
    run_case("timeunet_eval_k2_tame", "timeunet", "tame", 205, 215, 2, 4, 16, [4, 2], "eval", ctor=dict(K2))
    run_case("wtae_train_k2_tame", "wtae", "tame", 206, 216, 2, 4, 16, [4, 3], "train", ctor=dict(K2))
    run_case("wtae_eval_k6_tame", "wtae", "tame", 207, 217, 2, 4, 16, [4, 2], "eval", ctor=dict(K6))
    run_case("utae_eval_dwsep_k6_tame", "utae", "tame", 208, 218, 2, 5, 16, [5, 3], "eval",
             ctor=dict(K6, conv_type="depthwise_separable"))


if __name__ == "__main__":
    main()
