"""Record the bits apad_gemm writes through every piece csrc/gemm_shared.h holds (the 16-bit epilogue, the folded-LayerNorm row
statistics, the A-operand row decode and gather), on the GPU, BY RUNNING THE LIBRARY AS BUILT FROM THE COMMIT THAT IS TO BE PRESERVED
(APAD_LIB_PATH selects the binary):

    APAD_LIB_PATH=/path/to/libapadapter_hip.so python tests/golden/make_gemm_bits.py [OUT [REVISION]]   # writes gemm_bits.safetensors, or OUT

tests/test_gpu_gemm_bits.py imports CASES and run_case from here and asserts torch.equal against the file.  Inputs are not stored: they
come from a numpy.RandomState seeded per case.  Every case goes through ops.gemm / the typed wrappers; the shapes are the smallest at
which the piece can go wrong (ragged in M, N and K where the kernel allows it, two M-tiles).

What is stored of an output, viewed as [rows, cols] (record()): over ALL rows, two exact integer checksums per column of the bit patterns
-- their sum and their sum weighted by row number, modulo 2^32 -- so that a change of any single element changes the file's comparison;
and, as a sample to look at when a checksum differs, every KEEP-th row verbatim (the 128-tile case: every 61st).  Whole outputs would be
about three times tests/golden/step_bits.safetensors, the bound set for this file.

The ring cases (ops.set_gemm_ring(2)) are stored once: main() checks at recording time that the LDS-DMA ring form and the tiled form wrote
the same bits, and the test runs both forms against the one record.
"""
import os
import sys
import zlib

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
FIXTURE = os.path.join(HERE, "gemm_bits.safetensors")
DT16 = {"bf16": torch.bfloat16, "f16": torch.float16}
KEEP = 6


class Gen:
    """seeded inputs of one case, drawn in call order"""
    def __init__(self, seed, dev, dtype):
        self.rs, self.dev, self.dtype = np.random.RandomState(seed), dev, dtype

    def __call__(self, *shape, std=1.0, dtype=None):
        t = torch.from_numpy((self.rs.standard_normal(shape) * std).astype(np.float32))
        return t.to(self.dev, dtype or self.dtype)


# ---- the cases: fn(ops, g) -> {output name: tensor}; g(*shape) draws the next input ----
def _plain(ops, g, M=70, N=72, K=72):
    return g(M, K), g(N, K, std=0.1), g(N)


def c_plain(ops, g):
    x, w, b = _plain(ops, g)
    return {"out": ops.linear(x, w, b, residual=g(35, 72), residual_row_mod=35)}


def c_rg_table(ops, g):
    x, w, b = _plain(ops, g)
    step = torch.tensor([3], dtype=torch.int32, device=g.dev)
    return {"out": ops.linear(x, w, b, rowgroup_bias=g(5, 72), rows_per_group=1 << 40, step_ptr=step)}


def c_rg_group(ops, g):
    x, w, b = _plain(ops, g)
    return {"out": ops.linear(x, w, b, rowgroup_bias=g(2, 72), rows_per_group=35)}


def c_silu(ops, g):
    x, w, b = _plain(ops, g)
    return {"out": ops.linear(x, w, b, act="silu")}


def c_gelu(ops, g):
    x, w, b = _plain(ops, g)
    return {"out": ops.linear(x, w, b, act="gelu")}


def c_geglu(ops, g, K=72):
    return {"out": ops.linear(g(70, K), g(128, K, std=0.1), g(128), act="geglu")}  # N = 64


def c_rowstat_ln(ops, g, K=72, N2=72):
    """rowstat=True at N = 128 (+ residual), then the LayerNorm folded from those statistics at K = 128"""
    y = ops.linear(g(70, K), g(128, K, std=0.1), g(128), residual=g(70, 128), rowstat=True)
    z = ops.linear(y, g(N2, 128, std=0.1), g(N2), ln=(g(128), g(128), 1e-5))
    return {"y": y, "rowstat": ops.rowstat_of(y), "z": z}


def c_vt(ops, g):
    vt = torch.zeros(2, 2, 64, 40, dtype=g.dtype, device=g.dev)
    return {"vt": ops.linear_vt(g(70, 72), g(128, 72, std=0.1), 2, 35, 2, vt, bias=g(128))}


def c_qkv(ops, g, K=72):
    """OUT_QKV at C = 128 without and with the row-major v= copy: q, k, vt are the same bits in both (asserted), stored once"""
    x, w, b = g(70, K), g(384, K, std=0.1), g(384)
    outs = []
    for with_v in (False, True):
        q, k = (torch.empty(70, 128, dtype=g.dtype, device=g.dev) for _ in range(2))
        vt = torch.zeros(2, 2, 64, 40, dtype=g.dtype, device=g.dev)
        v = torch.empty(70, 128, dtype=g.dtype, device=g.dev) if with_v else None
        ops.linear_qkv(x, w, 2, 35, 2, q, k, vt, bias=b, v=v)
        outs.append((q, k, vt, v))
    assert all(torch.equal(a, c) for a, c in zip(outs[0][:3], outs[1][:3]))
    return dict(zip(("q", "k", "vt", "v"), outs[1]))


def c_linear2(ops, g, Cb=72, N=72):
    """the second source is the smaller batch: read modulo"""
    return {"out": ops.linear2(g(2, 35, 64), g(1, 35, Cb), g(N, 64 + Cb, std=0.1), g(N))}


def c_kgroup(ops, g):
    return {"out": ops.linear(g(70, 384), g(640, 384, std=0.05), g(640), residual=g(70, 640))}


def _conv(ops, g, B, H, W, Cin, Cout=72, **kw):
    old, ops.HCONV = ops.HCONV, False
    try:
        Bs = kw.get("src_batch_mod") or B
        out, Ho, Wo = ops.conv3x3(g(Bs, H * W, Cin), g(Cout, 9 * Cin, std=0.05), g(Cout), B, H, W, **kw)
    finally:
        ops.HCONV = old
    return {"out": out}


def c_conv_two_stage(ops, g):
    return _conv(ops, g, 2, 4, 4, 256)  # K = 2304: two LDS stages (and the FAST gather)


def c_conv_s2(ops, g):
    return _conv(ops, g, 2, 7, 5, 8, stride=2)


def c_conv_up(ops, g):
    return _conv(ops, g, 2, 4, 3, 8, up=(9, 7))


def c_conv_asym(ops, g):
    return _conv(ops, g, 2, 8, 6, 8, stride=2, asym_pad=True)


def c_conv_fast(ops, g):
    out = _conv(ops, g, 2, 7, 5, 64)
    out["shared_src"] = _conv(ops, g, 2, 7, 5, 64, src_batch_mod=1)["out"]
    return out


def c_conv1d_dil(ops, g, C=16):
    return {"out": ops.conv1d(g(2, 37, C), g(24, 3 * C, std=0.1), g(24), 3, dilation=3, pre_slope=0.1, residual=g(2, 37, 24))}


def c_conv1d_tr(ops, g, C=16):
    return {"out": ops.conv1d(g(2, 19, C), g(24, 4 * C, std=0.1), g(24), 4, transposed_stride=2)}


def c_conv1d_tanh(ops, g, C=16):
    return {"out": ops.conv1d(g(2, 37, C), g(8, 7 * C, std=0.1), g(8), 7, act="tanh")}


def c_patch16(ops, g, N=72):
    return {"out": ops.patch_embed(g(2, 16, 32, dtype=torch.float32), g(N, 256, std=0.1), g(N), g.dtype)}


def c_tile128(ops, g):
    """320 blocks of 128 rows, K = 1024, N = 24 (not the big-tile kernel's): the rule's 128-tile; the rows repeat 257 random ones"""
    M = 40900
    x = g(257, 1024)[torch.arange(M, device=g.dev) % 257]
    return {"out": ops.linear(x, g(24, 1024, std=0.05), g(24), residual=g(257, 24), residual_row_mod=257)}


# the ring's envelope wants K % 64 == 0 and whole N tiles: its own shapes, M = 70; each runs on the tiled kernel and on the ring
def c_r_plain(ops, g):
    return {"out": ops.linear(g(70, 128), g(128, 128, std=0.1), g(128), residual=g(35, 128), residual_row_mod=35)}


def c_r_geglu(ops, g):
    return c_geglu(ops, g, K=128)


def c_r_qkv(ops, g):
    return c_qkv(ops, g, K=128)


def c_r_rowstat_ln(ops, g):
    return c_rowstat_ln(ops, g, K=128, N2=128)


def c_r_linear2(ops, g):
    return c_linear2(ops, g, Cb=64, N=128)


# fp32 ("highest": the exact-f32 MFMA; "high": bf16x3), dims multiples of 4
def c_f_plain(ops, g):
    return {"out": ops.linear(g(37, 36), g(36, 36, std=0.1), g(36), residual=g(37, 36))}


def c_f_conv(ops, g):
    return _conv(ops, g, 2, 7, 5, 4, Cout=36, stride=2)


def c_f_conv1d_tr(ops, g):
    return c_conv1d_tr(ops, g, C=8)


def c_f_patch16(ops, g):
    return c_patch16(ops, g, N=36)


def c_f_acts(ops, g):
    x = g(37, 36)
    return {"relu": ops.linear(x, g(36, 36, std=0.1), g(36), act="relu"), "gelu_tanh": ops.linear(x, g(36, 36, std=0.1), g(36), act="gelu_tanh"),
            "geglu_tanh": ops.linear(x, g(64, 36, std=0.1), g(64), act="geglu_tanh")}


def c_f_vt(ops, g):
    vt = torch.zeros(2, 2, 32, 40, dtype=g.dtype, device=g.dev)
    return {"vt": ops.linear_vt(g(70, 36), g(64, 36, std=0.1), 2, 35, 2, vt, bias=g(64))}


def c_f_qkv(ops, g):
    q, k = (torch.empty(70, 64, dtype=g.dtype, device=g.dev) for _ in range(2))
    vt = torch.zeros(2, 2, 32, 40, dtype=g.dtype, device=g.dev)
    ops.linear_qkv(g(70, 36), g(192, 36, std=0.1), 2, 35, 2, q, k, vt, bias=g(192))
    return {"q": q, "k": k, "vt": vt}


TILED = [c_plain, c_rg_table, c_rg_group, c_silu, c_gelu, c_geglu, c_rowstat_ln, c_vt, c_qkv, c_linear2, c_kgroup, c_conv_two_stage, c_conv_s2,
         c_conv_up, c_conv_asym, c_conv_fast, c_conv1d_dil, c_conv1d_tr, c_conv1d_tanh, c_patch16, c_tile128]
RING = [c_r_plain, c_r_geglu, c_r_qkv, c_r_rowstat_ln, c_r_linear2, c_kgroup]
F32 = [c_f_plain, c_f_conv, c_f_conv1d_tr, c_f_patch16, c_f_acts, c_f_vt, c_f_qkv]
FN = {f.__name__[2:]: f for f in TILED + RING + F32}
# (function name, dtype or fp32 precision, ring mode)
CASES = [(f.__name__[2:], d, 0) for f in TILED for d in DT16]
CASES += [(f.__name__[2:], d, m) for f in RING for d in DT16 for m in (0, 2) if (f.__name__[2:], d, m) not in CASES]
CASES += [(f.__name__[2:], p, 0) for f in F32 for p in ("highest", "high")]


def fixture_key(case):
    """the tiled and the ring form of a case share one record"""
    return case[0] + "." + case[1]


def run_case(case, dev):
    """-> {output name: tensor on the device}"""
    from ap_adapter_amd import ops
    name, d, ring = case
    g = Gen(zlib.crc32(name.encode()), dev, DT16.get(d, torch.float32))
    old_ring, old_prec = ops.set_gemm_ring(ring), ops.get_float32_matmul_precision()
    try:
        if d not in DT16:
            ops.set_float32_matmul_precision(d)
        return FN[name](ops, g)
    finally:
        ops.set_gemm_ring(old_ring)
        ops.set_float32_matmul_precision(old_prec)


def record(case, out):
    """-> {fixture entry: CPU tensor}: what the file keeps of the outputs of one case"""
    keep = 61 if case[0] == "tile128" else KEEP
    rec = {}
    for name, t in out.items():
        t2 = t.reshape(-1, t.shape[-1])
        bits = t2.view(torch.int16 if t2.element_size() == 2 else torch.int32).to(torch.int64)
        rows = torch.arange(1, t2.shape[0] + 1, device=t.device)[:, None]
        key = fixture_key(case) + "." + name
        rec[key] = t2[::keep].cpu().contiguous().clone()
        rec[key + ".colsums"] = torch.stack([bits.sum(0), (bits * rows).sum(0)]).to(torch.int32).cpu()  # (wraps: modulo 2^32)
    return rec


def main(path=FIXTURE, revision="unknown"):
    from safetensors.torch import save_file
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    from ap_adapter_amd import _lib as L
    dev = torch.device("cuda:0")
    tensors = {}
    for case in CASES:
        for key, t in record(case, run_case(case, dev)).items():
            if key in tensors:  # the ring form: must be the tiled form's bits already recorded
                assert torch.equal(tensors[key], t), (case, key)
            tensors[key] = t
    save_file(tensors, path, metadata={"generator": "tests/golden/make_gemm_bits.py", "device": torch.cuda.get_device_name(0),
                                          "torch": torch.__version__, "cases": str(len(CASES)), "library_revision": revision,
                                          "library": os.path.basename(os.path.dirname(L.LIB_PATH)) + "/" + os.path.basename(L.LIB_PATH)})
    print("wrote", path, os.path.getsize(path), "bytes,", len(tensors), "tensors,", len(CASES), "cases")


if __name__ == "__main__":
    main(*sys.argv[1:3])
