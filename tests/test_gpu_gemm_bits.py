"""-m gpu: the bits apad_gemm writes through the pieces of csrc/gemm_shared.h (the 16-bit epilogue shared by the tiled and the ring
kernel, the folded-LayerNorm row statistics, the A-operand row decode and gather shared by the 16-bit and the fp32 kernels), against
tests/golden/gemm_bits.safetensors: what the separately written kernels of the commit before the header wrote, recorded on the device by
tests/golden/make_gemm_bits.py (whose CASES, run_case and record this module runs again).  torch.equal, every stored entry, every case."""
import os

import pytest
import torch
from safetensors.torch import load_file

import make_gemm_bits as MG
import make_step_bits as MS

pytestmark = pytest.mark.gpu

GOLD = load_file(MG.FIXTURE)


def test_fixture_is_small_and_holds_only_the_cases():
    assert os.path.getsize(MG.FIXTURE) <= os.path.getsize(MS.FIXTURE)
    assert {k.rsplit(".", 2 if k.endswith(".colsums") else 1)[0] for k in GOLD} == {MG.fixture_key(c) for c in MG.CASES}


@pytest.mark.parametrize("case", MG.CASES, ids=lambda c: "-".join(map(str, c)))
def test_gemm_bits_are_the_recorded_ones(dev, case):
    rec = MG.record(case, MG.run_case(case, dev))
    assert set(rec) == {k for k in GOLD if k.startswith(MG.fixture_key(case) + ".")}
    for key, t in rec.items():
        assert t.dtype == GOLD[key].dtype and torch.equal(t, GOLD[key]), (case, key)
