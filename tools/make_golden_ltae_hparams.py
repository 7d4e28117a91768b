"""Golden fixture of an L-TAE d_model away from the reference's default 256 (train.py:41; the model classes keep n_head = 16,
d_k = 4), from the imported reference models (oracle/make_golden.run_case).  Needs the reference sources on PYTHONPATH:

    PYTHONPATH=<reference checkout>:. python tools/make_golden_ltae_hparams.py

Writes tests/golden/*_h{n_head}m{d_model}k{d_k}_tame.npz; conftest.golden_names() picks it up.  U-TAE keeps d_model = 256
(utae.py:179 builds its L-TAE with mlp=[256,128]), so the fixture is a TimeUNet.  CPU only: the GPU suite reads the written
file, never this tool.
"""
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))

import torch  # noqa: E402

from oracle.make_golden import run_case  # noqa: E402


def main():
    torch.set_num_threads(8)
    run_case("timeunet_eval_h16m512k4_tame", "timeunet", "tame", 305, 315, 2, 4, 16, [4, 2], "eval",
             ctor=dict(n_head=16, d_model=512, d_k=4))


if __name__ == "__main__":
    main()
