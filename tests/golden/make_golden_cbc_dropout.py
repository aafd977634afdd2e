"""Records tests/golden/cbc_dropout.npz: outputs and gradients of the bf16 output-dropout cells of tests/test_sublayer_cbc.py (p = 0.3,
fixed key) on the call-by-call path, on an MI355X.  Run at the commit BEFORE the shared call-by-call driver (--root: a checkout of it;
AFFT_LIB may point it at this checkout's library, which that change leaves alone), twice: the second run with --compare FILE lists every
entry that did not come back bit for bit.

    python tests/golden/make_golden_cbc_dropout.py --root PARENT --out tests/golden/cbc_dropout.npz
    python tests/golden/make_golden_cbc_dropout.py --root PARENT --compare tests/golden/cbc_dropout.npz
"""
import argparse
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--root", default=ROOT)
    ap.add_argument("--out")
    ap.add_argument("--compare")
    a = ap.parse_args()
    sys.path[:0] = [os.path.abspath(a.root), os.path.join(ROOT, "tests"), HERE]
    import afft_amd
    from afft_amd import runtime as rt
    import test_sublayer_cbc as M
    rt.set_composite(False)
    afft_amd.set_precision("bf16")
    res = {}
    for cell in M.DROPOUT_CELLS:
        for k, v in M.run_cell(cell, torch.device("cuda:0")).items():
            res[cell["fn"] + "." + k] = v.numpy()
    if a.out:
        np.savez(a.out, **res)
        print(f"{len(res)} entries -> {a.out} ({os.path.dirname(afft_amd.__file__)})")
    if a.compare:
        z = np.load(a.compare)
        assert sorted(z.files) == sorted(res), "different entries"
        bad = [k for k in sorted(res) if not np.array_equal(z[k], res[k])]
        print(f"{len(res) - len(bad)} of {len(res)} entries equal to {a.compare} ({os.path.dirname(afft_amd.__file__)})" + "".join("\n  differs: " + k for k in bad))
        sys.exit(1 if bad else 0)


if __name__ == "__main__":
    main()
