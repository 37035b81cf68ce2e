"""Short, seeded runs of tools/fuzz_gemm_paths.py: random shapes through the GEMM entry points - on the split-f16 engine
with a mode forced per case, and on the exact-fp32 engine (mode 0) with a tile override drawn per case and backward
K-segments of any length."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), '..', 'tools'))


@pytest.mark.parametrize('seed', [3, 11])
def test_random_shapes_against_fp64(seed):
    import fuzz_gemm_paths
    assert fuzz_gemm_paths.run(seed, 30, verbose=False) == 0


@pytest.mark.parametrize('seed', [5, 17])
def test_random_shapes_on_the_exact_fp32_engine_against_fp64(seed):
    import fuzz_gemm_paths
    from insenticap_model_amd import ops
    try:
        assert fuzz_gemm_paths.run(seed, 30, verbose=False, engine='f32') == 0
    finally:
        ops.set_tile_override(-1)
        ops.set_h3_mode(1)
