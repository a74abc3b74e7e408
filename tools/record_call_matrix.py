#!/usr/bin/env python
"""Record tests/golden/engine_call_matrix.json: what every probe call returns at every engine state (tests/call_matrix.py).

The recording is the behaviour a change of the engine's call handling has to keep, so it is taken from the library built from the
commit BEFORE such a change, selected with Q3A_LIB as tools/ab_bench.sh does (keep that .so out of git):

    Q3A_BUILD_VARIANT=parent python -m qwen3_asr_rs_amd.build          # in a checkout of the parent's csrc
    Q3A_LIB=$PWD/qwen3_asr_rs_amd/lib/libq3asr_hip_parent.so python tools/record_call_matrix.py

tests/test_gpu_call_matrix.py runs the same driver and compares every row exactly; it has to pass on both libraries.
"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
OUT = os.path.join(ROOT, "tests", "golden", "engine_call_matrix.json")


def main():
    from call_matrix import run_matrix
    from qwen3_asr_rs_amd import _lib, synthetic
    rows = run_matrix(synthetic.write_checkpoint("/tmp/q3a_ckpt_tiny", "tiny", seed=1))
    out = sys.argv[1] if len(sys.argv) > 1 else OUT
    with open(out, "w") as f:
        f.write("[\n" + ",\n".join(json.dumps(r) for r in rows) + "\n]\n")  # one row per line
    print(f"{len(rows)} rows ({sum(r['rc'] != 0 for r in rows)} refusals) from {_lib.LIB_PATH} -> {out}")


if __name__ == "__main__":
    main()
