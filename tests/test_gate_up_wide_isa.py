"""The gate / up GEMV of the one-sequence chain with twelve waves per workgroup (csrc/k_gemv.hip gemv1_xp_kernel / gemv1_xp_body) in the
device assembly the build keeps, read with tools/isa_waits.py as tests/test_isa_hazards.py does.  CPU only: hipcc cross-compiles.

The workgroup's waves take roles behind one scalar branch at entry -- waves 0..3 request x and the four partial vectors of their columns
(5 requests) in front of their four weight chunks, waves 4..7 the norm weight (1), the others their weights only -- and each role is a
straight-line program: its requests must form one run in front of its first wait (a load under a branch that joins again in front of
further requests made hipcc wait at the join, twice: docs/HISTORY.md).  The descriptor must allow 12 x 64 threads at no more than 168
VGPRs (three waves per SIMD), use no scratch and preload the 14 dwords of the head."""
import importlib.util
import os
import re

import pytest

from qwen3_asr_rs_amd import build

needs_hipcc = pytest.mark.skipif(not build.have_hipcc(), reason=f"{build.HIPCC} not found: the device assembly cannot be produced here")

HANDOVER_PIECES, WEIGHT_CHUNKS, WAVES = 5, 4, 12  # a summing thread: x + 4 partial vectors; 2 rows x 2 k-iterations; waves per workgroup
XP = r"gemv1_xp_kernelILi2ELi2ELi12EEE"


def _isa_waits():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    spec = importlib.util.spec_from_file_location("isa_waits", os.path.join(root, "tools", "isa_waits.py"))
    iw = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(iw)
    return iw


@needs_hipcc
def test_hand_over_and_weights_are_requested_in_one_run():
    build.build(verbose=False)
    iw = _isa_waits()
    mine = [(k, iw.tokens(b)) for _, k, b in iw.kernels() if re.search(XP, k)]
    assert len(mine) == 1, [k for k, _ in mine]
    seq = mine[0][1]
    line = iw.compress(seq)
    print(f"{mine[0][0]}: {line}")
    # a role's stretch starts behind the previous role's last store (or at the kernel's entry) and holds one long run of requests; the
    # bias loads, which sit behind a test of the bias pointer as in every GEMV form, follow that run
    roles, i = [], 0
    while i < len(seq):
        if seq[i] != "G":
            i += 1
            continue
        j = i
        while j < len(seq) and seq[j] == "G":
            j += 1
        if j - i >= WEIGHT_CHUNKS:
            start = max([k for k in range(i) if seq[k] == "S"] or [-1]) + 1
            roles.append((j - i, [t for t in seq[start:i] if t.startswith("W")]))
        i = j
    print(f"request runs per role (in code order): {[n for n, _ in roles]}")
    assert len(roles) == 3
    assert sorted(n for n, _ in roles) == [WEIGHT_CHUNKS, 1 + WEIGHT_CHUNKS, HANDOVER_PIECES + WEIGHT_CHUNKS]
    assert all(not waits for _, waits in roles), "a wait in front of a role's requests"


@needs_hipcc
def test_descriptor_workgroup_size_scratch_and_preloaded_head():
    build.build(verbose=False)
    txt = open(build.isa_path("k_gemv.hip")).read()
    desc = re.search(r"\.amdhsa_kernel (\S*" + XP + r"\S*)\n(.*?)\.end_amdhsa_kernel", txt, re.S)
    assert desc, "no descriptor of the XP kernel"
    field = lambda k: int(re.search(r"\." + k + r"\s+(\d+)", desc.group(2)).group(1))  # noqa: E731
    meta = next(b for b in re.split(r"\n  - (?=\.agpr_count)", txt)[1:] if re.search(r"\.name:\s+" + re.escape(desc.group(1)) + r"\s", b))
    mfield = lambda k: int(re.search(r"\." + k + r":\s+(\d+)", meta).group(1))  # noqa: E731
    print(f"{desc.group(1)}: max_flat_workgroup_size {mfield('max_flat_workgroup_size')}, vgpr {field('amdhsa_next_free_vgpr')}, "
          f"scratch {field('amdhsa_private_segment_fixed_size')}, lds {field('amdhsa_group_segment_fixed_size')}, "
          f"preload {field('amdhsa_user_sgpr_kernarg_preload_length')}")
    assert mfield("max_flat_workgroup_size") == WAVES * 64
    assert field("amdhsa_private_segment_fixed_size") == 0 and mfield("vgpr_spill_count") == 0
    assert field("amdhsa_next_free_vgpr") <= 168  # 12 waves per workgroup: three per SIMD, 512 / 3 rounded down to the allocation unit of 8
    assert field("amdhsa_user_sgpr_kernarg_preload_length") == 14            # the head: five pointers, N, K, x_nparts, eps
