"""The knob forms of the segment attention live in processes of their own: Q3A_FATTN_NS and Q3A_FATTN_DMA are read once per process.
tests/test_gpu_seg_attn.py starts this file in a fresh interpreter with one of them set; it launches the named cases of
tests/seg_attn_ref.py through q3a_selftest_seg_attn_launch and writes the raw output buffers and the reported forms to an .npz.

    python tests/seg_attn_child.py OUT.npz CASE [CASE ...]
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for p in (HERE, os.path.dirname(HERE)):
    if p not in sys.path:
        sys.path.insert(0, p)


def main(out_path, names):
    import seg_attn_ref as R
    from qwen3_asr_rs_amd import _lib
    lib = _lib.load()
    by_name = dict(R.BY_NAME, **{c["name"]: c for c in R.grid_cases()})
    res = {}
    for name in names:
        c = by_name[name]
        raw, form = R.launch(lib, c, R.inputs(c))
        if raw is None:
            print(f"{name}: {form}", file=sys.stderr)
            return 2
        res[name + "|out"] = raw
        res[name + "|form"] = np.asarray([form[k] for k in R.FORM_FIELDS], np.int32)
    np.savez(out_path, **res)
    return 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], sys.argv[2:]))
