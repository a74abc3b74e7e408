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
# kernel instantiations per source: a change that adds or loses one says so here.  (395 before the step's logits processors each got a
# kernel of their own: k_repeat.hip 1 -> 2, k_sample.hip 5 -> 10, k_toplp.hip new with 3.)
KERNELS = {"k_align.hip": 15, "k_attn.hip": 7, "k_beam.hip": 27, "k_conv1.hip": 2, "k_dattn.hip": 14, "k_decode.hip": 8, "k_draft.hip": 1,
           "k_fattn.hip": 14, "k_gemm.hip": 27, "k_gemm16.hip": 34, "k_gemm256.hip": 4, "k_gemv.hip": 83, "k_mel.hip": 2, "k_norm.hip": 4,
           "k_ops.hip": 16, "k_peaks.hip": 5, "k_repeat.hip": 2, "k_sample.hip": 10, "k_skinny.hip": 126, "k_toplp.hip": 3}
KERNELS_IN_LIBRARY = 404


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
    counts = {}
    for src in build.SOURCES:
        if not src.endswith(".hip"):
            continue
        lengths, n = _descriptors(src)
        counts[src] = n
        assert len(lengths) == n, src  # every descriptor carries the directive
        for stem in CHAIN.get(src, []):
            mine = {k: v for k, v in lengths.items() if re.search(r"\d+" + stem + "I", k)}
            assert mine, (src, stem)
            short = {k: v for k, v in mine.items() if v < 8}
            assert not short, short
    assert counts == KERNELS, {k: (counts.get(k), KERNELS.get(k)) for k in set(counts) | set(KERNELS) if counts.get(k) != KERNELS.get(k)}
    assert sum(counts.values()) == KERNELS_IN_LIBRARY == sum(KERNELS.values())
