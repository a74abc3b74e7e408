"""Kernel-argument preload (qwen3_asr_rs_amd/build.py KERNARG_PRELOAD_FLAGS): every kernel of the one-sequence decode chain takes a
flat head of pointers and ints in front of its tail struct, and the compiler marks those dwords for preloading into SGPRs at wave
launch -- `.amdhsa_user_sgpr_kernarg_preload_length` in the kernel descriptor.  A kernel whose only parameter is a struct by value has
length 0 (the struct is a byref argument), so a signature that slides back to one shows up here.  CPU only: hipcc cross-compiles, and
the test reads that metadata directive of the assembly `python -m qwen3_asr_rs_amd.build` keeps, nothing else."""
import re

import pytest

from qwen3_asr_rs_amd import build

needs_hipcc = pytest.mark.skipif(not build.have_hipcc(), reason=f"{build.HIPCC} not found: the device assembly cannot be produced here")

# the kernels of the per-token chain at one sequence, and the source they live in
CHAIN = {"k_gemv.hip": ["gemv1_kernel", "gemv1_head_kernel", "lm_head_approx_kernel", "lm_head_approx_bias_kernel", "lm_head_rescore_kernel"],
         "k_dattn.hip": ["decode_attn_kernel"], "k_decode.hip": ["argmax_finalize_kernel"]}
KERNELS_IN_LIBRARY = 395  # instantiations in the library before the kernels' signatures changed: none added, none lost


def _descriptors(src):
    txt = open(build.isa_path(src)).read()
    return {m.group(1): int(m.group(2)) for m in
            re.finditer(r"\.amdhsa_kernel (\S+)\n(?:(?!\.end_amdhsa_kernel).)*?\.amdhsa_user_sgpr_kernarg_preload_length (\d+)", txt, re.S)}, \
        len(re.findall(r"^\s*\.amdhsa_kernel ", txt, re.M))


@needs_hipcc
def test_the_flag_is_part_of_the_hip_build():
    assert "-amdgpu-kernarg-preload-count=14" in build.HIP_FLAGS and "-mllvm" in build.HIP_FLAGS
    assert build.HIP_FLAGS.count("-amdgpu-kernarg-preload-count=14") == 1  # an LLVM option may be given once


@needs_hipcc
def test_every_kernel_of_the_one_sequence_chain_preloads_its_head():
    build.build(verbose=False)
    total = 0
    for src in build.SOURCES:
        if not src.endswith(".hip"):
            continue
        lengths, n = _descriptors(src)
        total += n
        assert len(lengths) == n, src  # every descriptor carries the directive
        for stem in CHAIN.get(src, []):
            mine = {k: v for k, v in lengths.items() if re.search(r"\d+" + stem + "I", k)}
            assert mine, (src, stem)
            short = {k: v for k, v in mine.items() if v < 8}
            assert not short, short
    assert total == KERNELS_IN_LIBRARY, total
