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
    instead of as stale data of an earlier test.  (Only memory the allocator holds and no live tensor uses is written.)

    Unreachable reference cycles are collected first: the snapshot below builds thousands of Python objects, which can start a
    collection of its own, and a tensor that one frees AFTER the snapshot was taken leaves a block of stale data that is neither
    live nor filled -- the next small torch.empty then returns it."""
    import ctypes
    import gc
    gc.collect()
    torch.cuda.synchronize(dev)
    lib = _hip_runtime()
    stream = torch.cuda.current_stream(dev).cuda_stream
    for seg in torch.cuda.memory_snapshot():
        if seg.get("device", dev.index or 0) != (dev.index or 0):
            continue
        addr = seg["address"]
        for blk in seg["blocks"]:
            # (after the synchronize no kernel uses a freed block any more, whether or not the allocator has retired its events yet)
            if blk["state"] != "active_allocated" and blk["size"] >= 4:
                rc = lib.hipMemsetD32Async(ctypes.c_void_p(addr), NAN_WORD, blk["size"] // 4, ctypes.c_void_p(stream))
                assert rc == 0, f"hipMemsetD32Async: error {rc}"
            addr += blk["size"]
    torch.cuda.synchronize(dev)


def _nan_bits(dtype):
    """(integer view dtype, the NAN_WORD pattern at that width) of a storage dtype"""
    size = torch.empty((), dtype=dtype).element_size()
    if size == 2:
        return torch.int16, NAN_WORD & 0xFFFF
    if size == 4:
        return torch.int32, NAN_WORD
    raise TypeError(f"no NaN fill pattern for {dtype}")


def nan_buffer(n, dtype, device):
    """a flat [n] tensor of ``dtype`` whose every element is the NAN_WORD pattern"""
    idt, word = _nan_bits(dtype)
    return torch.full((n,), word, dtype=idt, device=device).view(dtype)


# the largest row tile of any kernel in csrc/ (cgemm.hip CBM = 256, hconv.hip BM = 256): a whole-tile over-run of any launch
# lands inside a guard of this many rows
GUARD_ROWS = 256


def guarded(rows, cols, dtype, device, ld=None, guard_rows=GUARD_ROWS):
    """(view, check): ONE flat allocation [guard_rows | rows | guard_rows] x ld (ld >= cols) whose every byte is the NAN_WORD
    pattern, the [rows, cols] strided view of its middle, and a check() to call after the launches that write the view.  check()
    asserts that both guards and the pad columns cols..ld are bit-identical to the fill and that every interior element is finite;
    its message names the first offending (row, column) in the view's coordinates (front guard: negative rows, back guard: rows
    >= ``rows``, pad: columns >= ``cols``) and says whether it is a stray write or a missing write."""
    ld = cols if ld is None else ld
    assert ld >= cols > 0 and rows > 0 and guard_rows >= 0
    idt, word = _nan_bits(dtype)
    buf = nan_buffer((rows + 2 * guard_rows) * ld, dtype, device)
    view = buf[guard_rows * ld:(guard_rows + rows) * ld].view(rows, ld)[:, :cols]

    def first(mask):
        i = int(mask.reshape(-1).to(torch.uint8).argmax())
        return i // mask.shape[1], i % mask.shape[1]

    def check(what=""):
        bits = buf.view(idt).view(rows + 2 * guard_rows, ld).cpu()
        vals = buf.view(rows + 2 * guard_rows, ld).cpu()
        tag = f"{what}: " if what else ""
        regions = (("front guard", bits[:guard_rows], -guard_rows, 0), ("back guard", bits[guard_rows + rows:], rows, 0),
                   ("pad columns", bits[guard_rows:guard_rows + rows, cols:], 0, cols))
        for name, reg, r0, c0 in regions:
            bad = reg != word
            if bool(bad.any()):
                r, c = first(bad)
                raise AssertionError(f"{tag}stray write in the {name} at (row {r + r0}, column {c + c0}) of a [{rows}, {cols}] result "
                                     f"(ld {ld}): {int(bad.sum())} element(s) changed")
        inner = vals[guard_rows:guard_rows + rows, :cols]
        bad = ~torch.isfinite(inner.float())
        if bool(bad.any()):
            r, c = first(bad)
            unwritten = int(bits[guard_rows + r, c]) == word
            kind = "missing write (still the fill pattern)" if unwritten else f"non-finite value written ({float(inner[r, c])})"
            raise AssertionError(f"{tag}{kind} at (row {r}, column {c}) of a [{rows}, {cols}] result (ld {ld}): "
                                 f"{int(bad.sum())} non-finite element(s)")

    return view, check


def poisoned_input(t, ld, tail_rows=GUARD_ROWS):
    """the dense 2-D operand ``t`` embedded in a [rows + tail_rows, ld] buffer whose pad columns and rows after the last are NaN
    (NAN_WORD); returns the [rows, cols] strided view.  A kernel that lets bytes outside its operand reach the result (a K tail
    masked by multiplication, a row past M) gives NaN."""
    rows, cols = t.shape
    assert ld >= cols
    buf = nan_buffer((rows + tail_rows) * ld, t.dtype, t.device).view(rows + tail_rows, ld)
    view = buf[:rows, :cols]
    view.copy_(t)
    return view
