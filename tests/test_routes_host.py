"""The attention sites' route decision (processors.route) on the host: every golden case, entered plainly and the way the block enters it, in
bf16, f16 and fp32, against the hand-kept envelope sets of tests/golden/cases.py.  Needs neither a GPU nor the built library."""
import functools

import pytest
import torch

from cases import (BLOCK_CASES, CASES, FUSED_ENVELOPE, HS_ENVELOPE, LN_EPS, R4_BLOCK_CASES, R4_CASES, R5_BLOCK_CASES, R5_CASES, R6_BLOCK_CASES,
                   ROWS_ENVELOPE, SATTN_ENVELOPE, make_inputs)

PLAIN = CASES + R4_CASES + R5_CASES
BLOCK = BLOCK_CASES + R4_BLOCK_CASES + R5_BLOCK_CASES + R6_BLOCK_CASES
ALL = PLAIN + BLOCK
DTYPES = [torch.bfloat16, torch.float16, torch.float32]


def expected(case, dtype, off=()):
    """the route by the hand-kept sets; ``off``: routes a switch has closed (their cases fall to the chain)"""
    if dtype == torch.float32:
        return "chain"
    for r, names in (("fused", FUSED_ENVELOPE), ("rows", ROWS_ENVELOPE), ("hs", HS_ENVELOPE), ("sattn", SATTN_ENVELOPE)):
        if case["name"] in names:
            return "chain" if r in off else r
    return "chain"


@functools.lru_cache(maxsize=None)
def _inputs(name):
    return make_inputs(next(c for c in ALL if c["name"] == name))


def asked(case, dtype):
    """build the Attention module and its processor on the CPU the way the GPU tests do, and ask the router what the call would run"""
    from ap_adapter_amd import AttnProcessor2_0, IPAttnProcessor2_0, processors as P
    from ap_adapter_amd.unet import Attention
    t = _inputs(case["name"])
    C_, X, heads = case["C"], case["X"], case["heads"]
    attn = Attention(C_, None if case["kind"] == "self" else X, heads, C_ // heads)
    if case["kind"] == "ip":
        proc = IPAttnProcessor2_0(hidden_size=C_, name="golden", cross_attention_dim=X, num_tokens=case["num_tokens"], scale=case["scale"])
    else:
        proc = AttnProcessor2_0()
    attn.set_processor(proc)
    attn = attn.to(dtype).requires_grad_(False)
    hs = t["hs"].to(dtype)
    residual, ln = (hs, (t["ln_g"].to(dtype), t["ln_b"].to(dtype), LN_EPS)) if case["block"] else (None, None)
    hs, residual, _ = P._as_tokens(hs, residual)  # (the 4-D entry hands the router its tokens)
    assert tuple(hs.shape) == (case["B"], case["N"], C_)
    masked = t["mask_bias"] is not None
    if case["kind"] == "self":
        return P.route("self", attn, hs, residual, ln, masked=masked)
    ehs = t["ehs"] if t["ehs"].dim() == 3 else t["ehs"].unsqueeze(0)
    L1, L2 = (case["L"], 0) if case["kind"] == "cross" else (case["num_tokens"], case["L"] - case["num_tokens"])
    assert (L1, L2) == proc._lengths(ehs)
    return P.route(proc.kind, attn, hs, residual, ln, L1, L2, masked, ehs.shape[0] == hs.shape[0])


def test_the_case_table_is_the_one_the_gpu_tests_run():
    assert len(PLAIN) == 26 and len(BLOCK) == 31
    names = {c["name"] for c in ALL}
    assert len(names) == len(ALL) and (FUSED_ENVELOPE | ROWS_ENVELOPE | HS_ENVELOPE | SATTN_ENVELOPE) <= names
    assert all(c["block"] for c in BLOCK) and not any(c["block"] for c in PLAIN)


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "f16", "f32"])
@pytest.mark.parametrize("case", ALL, ids=[c["name"] for c in ALL])
def test_route_of_every_golden_case(case, dtype):
    assert asked(case, dtype) == expected(case, dtype)


@pytest.mark.parametrize("switch,off", [("P.USE_FUSED_XATTN", ("fused", "rows")), ("ops.HS_ATTN", ("hs",)), ("ops.SATTN_FUSED", ("sattn",))])
def test_a_switch_closes_its_routes_and_no_other(switch, off, monkeypatch):
    from ap_adapter_amd import ops, processors as P
    mod, attr = switch.split(".")
    monkeypatch.setattr({"P": P, "ops": ops}[mod], attr, False)
    for dtype in DTYPES[:2]:
        for case in ALL:
            got = asked(case, dtype)
            assert got not in off and got == expected(case, dtype, off), (case["name"], dtype, got)


def test_the_router_launches_nothing(monkeypatch):
    """it reads shapes, dtypes, strides and module attributes: with the library unreachable it still answers"""
    from ap_adapter_amd import _lib

    def no_library(*a, **kw):
        raise AssertionError("processors.route called into the library")

    monkeypatch.setattr(_lib, "lib", no_library)
    for case in ALL:
        assert asked(case, torch.bfloat16) == expected(case, torch.bfloat16)
