import torch
import torch.utils._python_dispatch
import torch.utils._pytree


def rel_err(out, ref):
    """max-abs error relative to the reference's max magnitude"""
    ref = ref.detach().float()
    return float((out.detach().float().cpu() - ref.detach().cpu()).abs().max() / ref.abs().max().clamp_min(1e-12))


class PerOpRounding(torch.utils._python_dispatch.TorchDispatchMode):
    """Runs fp32 torch code the way a 16-bit PyTorch pipeline runs it: every aten op computes in fp32 and its fp32
    outputs are rounded to ``dtype`` (what torch's half / bfloat16 kernels do: fp32 accumulate inside the op, one
    rounding per op output).  Under this mode the fp32 oracle chain becomes the SAME-PRECISION reference of the HIP
    path: 'the reference pipeline at this storage type'."""

    def __init__(self, dtype):
        super().__init__()
        self.dtype = dtype

    def __torch_dispatch__(self, func, types, args=(), kwargs=None):
        out = func(*args, **(kwargs or {}))
        rnd = lambda t: t.to(self.dtype).float() if isinstance(t, torch.Tensor) and t.dtype == torch.float32 else t
        return torch.utils._pytree.tree_map(rnd, out)


def q(t, dtype):
    """round a fp32 CPU tensor to the storage dtype and back (so oracle and HIP path see the same operand bits)"""
    return t.to(dtype).float()


# float32 = the fp32 precision mode (exact-f32 MFMA): only the summation order differs from the oracle
TOL = {torch.bfloat16: 2e-2, torch.float16: 3e-3, torch.float32: 1e-5}


_FULL_UNET = []


def full_unet(scale):
    """a fresh fp32 CPU copy of the AudioLDM2-large UNet (718 M parameters) with the adapter installed and the synthetic init the
    full-geometry tests share (seed 100, bias_std 0.01): built once per process, deep-copied per test (construction + init is ~15 s)"""
    import copy
    import ap_adapter_amd as A
    from ap_adapter_amd.synthetic import init_synthetic_
    if not _FULL_UNET:
        u = A.AudioLDM2UNet2DConditionModel()
        A.install_ap_adapter(u, None, scale=0.55)
        init_synthetic_(u, 100, bias_std=0.01)
        _FULL_UNET.append(u)
    u = copy.deepcopy(_FULL_UNET[0])
    for p in u.attn_processors.values():
        if hasattr(p, "to_k_ip"):
            p.scale = scale
    return u


def exact_operand(*shape, seed=0, std=1.0, shift=None):
    """fp32 N(0, std) (+ ``shift``, broadcast), rounded to bf16 and flushed to zero below 2^-14: every value is then exact in bf16,
    f16 and fp32, so the three precision modes and an fp64 reference all see the same numbers"""
    t = torch.randn(*shape, generator=torch.Generator().manual_seed(seed)) * std
    if shift is not None:
        t = t + shift
    t = t.to(torch.bfloat16).float()
    return torch.where(t.abs() < 2.0 ** -14, torch.zeros_like(t), t)


def block_rel_err(out, ref, nblocks):
    """(worst, index) of the max-abs error of each of ``nblocks`` equal blocks relative to that block's own max|ref| (the leading
    dims of ``out`` / ``ref`` must enumerate the blocks).  A block whose reference is all zero must be exactly zero: its error is
    0 or inf."""
    e = (out.detach().double().cpu() - ref.detach().double().cpu()).reshape(nblocks, -1).abs().amax(1)
    m = ref.detach().double().cpu().reshape(nblocks, -1).abs().amax(1)
    r = torch.where(m > 0, e / m.clamp_min(1e-300), torch.where(e > 0, torch.full_like(e, float("inf")), torch.zeros_like(e)))
    i = int(r.argmax())
    return float(r[i]), i


_HIP = []


def _hip_runtime():
    import ctypes
    if not _HIP:
        path = None
        with open("/proc/self/maps") as f:  # the HIP runtime torch already loaded
            for line in f:
                if "libamdhip64.so" in line:
                    path = line.split()[-1]
                    break
        lib = ctypes.CDLL(path or "libamdhip64.so")
        lib.hipMemsetD32Async.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
        lib.hipMemsetD32Async.restype = ctypes.c_int
        _HIP.append(lib)
    return _HIP[0]


# one 32-bit word that is a NaN as fp32 and whose two halves are NaNs as bf16 and as f16
NAN_WORD = 0x7FFF7FFF


def nan_fill_free(dev):
    """Fill every free block of torch's caching allocator on ``dev`` with NaN (NAN_WORD).  Outputs and scratch buffers the next
    launches allocate come from these blocks, so an element, pad column or scratch entry a kernel fails to write reads as NaN
    instead of as stale data of an earlier test.  (Only memory the allocator holds and no live tensor uses is written.)"""
    import ctypes
    torch.cuda.synchronize(dev)
    lib = _hip_runtime()
    stream = torch.cuda.current_stream(dev).cuda_stream
    for seg in torch.cuda.memory_snapshot():
        if seg.get("device", dev.index or 0) != (dev.index or 0):
            continue
        addr = seg["address"]
        for blk in seg["blocks"]:
            if blk["state"] == "inactive" and blk["size"] >= 4:
                rc = lib.hipMemsetD32Async(ctypes.c_void_p(addr), NAN_WORD, blk["size"] // 4, ctypes.c_void_p(stream))
                assert rc == 0, f"hipMemsetD32Async: error {rc}"
            addr += blk["size"]
    torch.cuda.synchronize(dev)
