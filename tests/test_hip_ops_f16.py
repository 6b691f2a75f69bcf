"""The per-kernel parity suite against the fp16 build of the library (libcrg_hip_f16.so, CRG_HALF=f16).

The library is chosen when cremage_amd is imported, so the fp16 run is ONE fresh child process: tests/test_hip_ops.py,
tests/test_half_type_edges.py, tests/test_batched_gemm_gpu.py (all generic over the process's half type, fp16 bounds = bf16
bounds / 8), tests/test_exact_gpu.py (bitwise on exact operands: no bound to scale, the tie offset follows the type) and
tests/test_attention_exact_gpu.py (exact softmaxes: bitwise in either type; its five knob runs are grandchildren, one at a time) plus the two fp32-class VAE goldens of tests/test_hip_models.py, whose three-pass convs then run on fp16 planes.  The child's first test establishes that it
really runs the fp16 library (test_half_type_edges.py::test_library_of_this_process_half_type).  test_linear_ring_gemm starts a
grandchild that inherits CRG_HALF: at most three processes hold the GPU.

Measured on MI355X: the child takes 40 s for its 777 cases, 1.2 s of them for the 45 of tests/test_batched_gemm_gpu.py, about 6 s
for the 57 of tests/test_exact_gpu.py, most of that their fp64 CPU references, and 13 s for the 272 of
tests/test_attention_exact_gpu.py when that file runs alone (the whole `-m gpu` run: 253 s for 1709 cases; the
suite's limit is 900 s), so nothing is deselected; a
parametrisation that had to be would be listed in DESELECT with its seconds, and the count below compares against the selection minus
that list.

Largest fp16 figure seen per test function against its bound (MI355X; `pytest -rP` prints every figure, `[fig]` lines):
  test_linear_shapes                                  rel-L2    2.09e-04 / 7.50e-04  (0.28)
  test_linear_transposed_range                        rel-L2    2.08e-04 / 7.50e-04  (0.28)
  test_layernorm_as_gemm_epilogue                     rel-L2    2.08e-04 / 7.50e-04  (0.28)
  test_linear_batched_tokens_and_f32_out              rel-L2    2.65e-07 / 5.00e-05  (0.01)
  test_geglu                                          rel-L2    2.08e-04 / 7.50e-04  (0.28)
  test_ln_linear                                      rel-L2    2.13e-04 / 7.50e-04  (0.28)
  test_row_resident_gemm_without_layernorm            rel-L2    2.08e-04 / 7.50e-04  (0.28)
  test_ln_linear_transposed_v                         rel-L2    2.08e-04 / 7.50e-04  (0.28)
  test_linear_transposed                              rel-L2    2.05e-04 / 7.50e-04  (0.27)
  test_conv2d                                         rel-L2    2.10e-04 / 7.50e-04  (0.28)
  test_conv2d_tile_configs                            rel-L2    2.07e-04 / 7.50e-04  (0.28)
  test_split_planes_path                              max-abs   1.07e-05 / 4.96e-04  (0.02)
  test_conv_rowhalo_shapes                            rel-L2    2.10e-04 / 7.50e-04  (0.28)
  test_conv_256_pixel_tile_shapes                     rel-L2    2.08e-04 / 7.50e-04  (0.28)
  test_conv_gn_fused                                  rel-L2    2.10e-04 / 7.50e-04  (0.28)
  test_conv_rowhalo_upsample                          rel-L2    2.07e-04 / 7.50e-04  (0.28)
  test_conv_rowhalo_planes                            max-abs   8.02e-06 / 3.13e-04  (0.03)
  test_conv_planes_gn_stats                           max-abs   1.33e-06 / 1.00e-04  (0.01)
  test_conv_unet_shapes                               rel-L2    2.07e-04 / 7.50e-04  (0.28)
  test_conv_small_four_pixels_per_thread              rel-L2    2.07e-04 / 7.50e-04  (0.28)
  test_conv_small                                     rel-L2    2.99e-04 / 7.50e-04  (0.40)
  test_group_norm                                     rel-L2    2.11e-04 / 7.50e-04  (0.28)
  test_group_norm_production_shapes                   rel-L2    2.09e-04 / 7.50e-04  (0.28)
  test_gn_stats_side_channel                          rel-L2    2.10e-04 / 7.50e-04  (0.28)
  test_gn_stats_concat_pair                           rel-L2    2.09e-04 / 7.50e-04  (0.28)
  test_gn_tile_partials                               rel-L2    2.09e-04 / 7.50e-04  (0.28)
  test_group_norm_concat                              rel-L2    2.09e-04 / 7.50e-04  (0.28)
  test_layer_norm                                     rel-L2    2.10e-04 / 7.50e-04  (0.28)
  test_softmax_rows                                   max-abs   8.94e-08 / 4.25e-05  (0.00)
  test_flash_attention                                rel-L2    3.62e-04 / 1.25e-03  (0.29)
  test_flash_attention_row_major_v                    rel-L2    2.78e-04 / 1.25e-03  (0.22)
  test_flash_attention_row_major_v_spiky_rows         rel-L2    1.85e-04 / 1.25e-03  (0.15)
  test_flash_attention_lds_dma_form                   rel-L2    3.82e-04 / 1.25e-03  (0.31)
  test_flash_attention_few_keys_kernel                rel-L2    2.61e-04 / 1.25e-03  (0.21)
  test_flash_attention_large_logits                   rel-L2    1.87e-03 / 2.50e-03  (0.75)
  test_flash_attention_spiky_rows                     rel-L2    1.91e-04 / 1.25e-03  (0.15)
  test_unfused_attention                              rel-L2    2.94e-04 / 1.25e-03  (0.24)
  test_unfused_attention_query_chunks_with_tail       rel-L2    2.92e-04 / 1.25e-03  (0.23)
  test_layout_and_elementwise                         rel-L2    2.35e-04 / 7.50e-04  (0.31)
  test_split_planes_reproduce_small_and_large_values  err/bound 1.00e+00 / 1.00e+00  (1.00)
  test_fp32_class_conv_small_magnitudes               rel-L2    3.40e-08 / 4.74e-07  (0.07)
  test_fp32_class_linear_small_magnitudes             rel-L2    3.18e-08 / 4.36e-07  (0.07)
  test_group_norm_split_feeds_fp32_class_conv         rel-L2    3.04e-08 / 3.57e-07  (0.09)
  test_conv_top_of_range                              rel-L2    2.09e-04 / 7.50e-04  (0.28)
  test_linear_top_of_range                            rel-L2    2.09e-04 / 7.50e-04  (0.28)
  test_group_norm_top_of_range                        rel-L2    2.10e-04 / 7.50e-04  (0.28)
  test_attention_crowd_of_improbable_keys             worst row 2.15e-04 / 1.25e-03  (0.17)
  test_few_keys_kernel_large_logits                   rel-L2    9.02e-05 / 2.50e-03  (0.04)
  test_layernorm_epilogue_large_offset                rel-L2    6.97e-04 / 7.50e-04  (0.93)
  test_layernorm_two_pass_large_offset                rel-L2    2.09e-04 / 7.50e-04  (0.28)
  test_raw_batched_gemm                               rel-L2    2.10e-04 / 7.50e-04  (0.28)
  test_linear_transposed_batched                      rel-L2    2.08e-04 / 7.50e-04  (0.28)
  test_unfused_attention_batched                      rel-L2    1.58e-05 / 5.00e-05  (0.32)
  test_unfused_attention_finite_garbage_in_v_pads     rel-L2    2.65e-04 / 1.25e-03  (0.21)
  test_softmax_rows_strided                           rel-L2    1.90e-04 / 7.50e-04  (0.25)
fp16 subnormals survive the conversions, the LDS-DMA path and the _f16 matrix instructions (fp32-class and crowd-attention rows:
at the 'subnormals kept' emulation, 20x to 200x below the 'flushed' one).  test_unfused_attention_batched's largest figure is the
fp32-class attention over 1536 keys (6.7e-6 on bf16 planes): probabilities near 1 / 1536 sit at the bottom of fp16's normal range, where
the lo plane of P has only subnormal steps left.  The one finding: test_layernorm_epilogue_large_offset
(GEGLU, offset 100 sigma) was at 9.8e-4 before the fp16 build folded the row statistics in fp64 (gemm_shared.h ln_row_coeffs).
"""
import os
import re
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu

SELECTION = ["tests/test_hip_ops.py", "tests/test_half_type_edges.py", "tests/test_batched_gemm_gpu.py", "tests/test_exact_gpu.py",
             "tests/test_attention_exact_gpu.py", "tests/test_hip_models.py::test_vae_sd15_full_decode_pixels", "tests/test_hip_models.py::test_vae_sd15_full_encode"]
DESELECT = []  # node ids (individual parametrisations only), each with its measured seconds
CHILD_TIME_LIMIT = 80  # seconds: about twice the measured 40


def _pytest(extra, timeout):
    from tests.conftest import REPO
    env = dict(os.environ, CRG_HALF="f16")
    cmd = [sys.executable, "-m", "pytest", *SELECTION, "-m", "gpu", "-q", "-p", "no:cacheprovider"]
    for d in DESELECT:
        cmd += ["--deselect", d]
    return subprocess.run(cmd + extra, cwd=REPO, env=env, capture_output=True, text=True, timeout=timeout)


def test_op_suite_against_the_fp16_library():
    c = _pytest(["--collect-only"], 300)  # collects only: no GPU call (the test files make none at import)
    m = re.search(r"^(\d+)(?:/\d+)? tests? collected", c.stdout, re.M)
    assert c.returncode == 0 and m, c.stdout[-3000:] + c.stderr[-3000:]
    collected = int(m.group(1))
    assert collected >= 351 + 2 + 45 + 57 + 272  # + tests/test_batched_gemm_gpu.py + tests/test_exact_gpu.py + tests/test_attention_exact_gpu.py
    r = _pytest(["-rs"], CHILD_TIME_LIMIT)  # started once: a failure is shown, not retried
    tail = r.stdout[-6000:] + r.stderr[-3000:]
    assert r.returncode == 0, tail
    summary = [ln for ln in r.stdout.splitlines() if re.search(r"\b\d+ passed\b", ln)][-1]
    print(f"\n[parity] fp16 library, {collected} cases collected: {summary.strip()}")
    counts = {k: int(n) for n, k in re.findall(r"(\d+) (passed|failed|skipped|errors?|xfailed|xpassed)", summary)}
    gn_tile_off = os.environ.get("CRG_GN_TILE", "1") == "0"  # test_gn_tile_partials skips itself then (as in the bf16 run)
    skipped = counts.pop("skipped", 0)
    assert skipped == (1 if gn_tile_off else 0), tail
    if skipped:
        assert re.search(r"SKIPPED \[1\] tests/test_hip_ops\.py:\d+: CRG_GN_TILE=0", r.stdout), tail
    assert counts == {"passed": collected - skipped}, (counts, collected, tail)
