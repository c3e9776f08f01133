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


# ---- integer operands: the linear kernels held to every bit (tests/exact_cases.py, test_gpu_exact_linear.py) ----
# With small-integer operands every product and partial sum of a linear kernel is an integer below 2^24, so fp32 accumulation is exact
# in ANY order (tile shape, K groups, ring stages, wave layout) and the result is a known integer: the kernel must store that integer
# correctly rounded.  Nothing here is measured on a kernel: the amplitudes follow from the formats, the conditions are checked on the
# fp64 reference.
DTYPE_MAX = {torch.bfloat16: 3.3895313892515355e38, torch.float16: 65504.0, torch.float32: 3.4028234663852886e38}


def int_operand(*shape, amp, seed, density=1.0):
    """fp32 integers uniform in [-amp, amp], each kept with probability ``density`` (else 0)"""
    g = torch.Generator().manual_seed(seed)
    t = torch.randint(-int(amp), int(amp) + 1, shape, generator=g).float()
    if density < 1.0:
        t = t * (torch.rand(shape, generator=g) < density).float()
    return t


def exact_case(K, dtype, tier):
    """(amp_x, amp_w, density_w) of a reduction of length K.
    Tier "A" (representable): x in [-2, 2], w in {-1, 0, 1} at density min(1, 36^2 / (2K)): the accumulator's sigma is about
    sqrt(K * 2 * density * 2/3) <= 30, so |acc| stays below 256 = what bf16 holds exactly (checked per case by assert_exact_conditions).
    Tier "B" (rounded; 16-bit only): x and w dense in [-a, a], a the smallest integer with a (a + 1) / 3 * sqrt(K) >= 600 (bf16) or 5000
    (f16): sigma of the outputs, far above the exactly-held range (256 / 2048) and far below the format's maximum."""
    if tier == "A":
        return 2, 1, min(1.0, 36.0 ** 2 / (2.0 * K))
    assert tier == "B" and dtype in (torch.bfloat16, torch.float16), (tier, dtype)
    target = 600.0 if dtype == torch.bfloat16 else 5000.0
    a = 1
    while a * (a + 1) / 3.0 * K ** 0.5 < target:
        a += 1
    return a, a, 1.0


def rne(t64, dtype):
    """an fp64 tensor of integers below 2^24 -> ``dtype``, round-to-nearest-even: the fp32 step is exact, the second is torch's rounding"""
    return t64.float().to(dtype)


def unrepresentable_and_ties(t64, dtype):
    """(fraction of elements ``dtype`` does not hold exactly, fraction that lie exactly half way between two neighbours)"""
    r = rne(t64, dtype).double()
    off = r != t64
    mirror = 2.0 * t64 - r  # the neighbour on the other side, if the element is a tie (else a number the format does not hold)
    tie = off & (rne(mirror, dtype).double() == mirror)
    n = max(t64.numel(), 1)
    return float(off.sum()) / n, float(tie.sum()) / n


def assert_exact_conditions(ref, intermediates, dtype, tier, K, amp_x, amp_w, side=()):
    """the conditions under which a linear kernel's output is determined in every bit, asserted on the fp64 reference alone (never on a
    kernel's output).  ref: the value the final rounding sees (a tensor, or a list of them); intermediates: the accumulator and
    every value a kernel may round on the way (acc + bias, ...); side: fp32 side outputs (row statistics)."""
    refs = list(ref) if isinstance(ref, (list, tuple)) else [ref]
    for t in refs + list(intermediates) + list(side):
        assert t.dtype == torch.float64 and torch.equal(t, t.round()), "not an integer"
    assert K * amp_x * amp_w < 2 ** 24, (K, amp_x, amp_w)
    top = max(float(t.abs().max()) for t in refs + list(intermediates))
    if tier == "A":
        assert top <= 256, f"max |value| {top} leaves the range bf16 holds exactly"
        for t in side:
            assert float(t.abs().max()) < 2 ** 24
    else:
        assert tier == "B" and dtype in (torch.bfloat16, torch.float16)
        assert not side, "tier B has no exact side outputs"
        assert top < DTYPE_MAX[dtype] / 2 and top < 2 ** 24, top
        for t in refs:
            off, tie = unrepresentable_and_ties(t, dtype)
            assert off >= 0.25 and tie >= 0.10, f"only {off:.1%} of the outputs are rounded, {tie:.1%} are ties"


def assert_bits_equal(out, expected, what=""):
    """torch.equal on the bit patterns; the message names the first differing (row, column) of the [-1, last dim] view"""
    assert out.dtype == expected.dtype and tuple(out.shape) == tuple(expected.shape), (what, out.dtype, expected.dtype, tuple(out.shape), tuple(expected.shape))
    idt = torch.int16 if out.element_size() == 2 else torch.int32
    a, e = out.detach().cpu().contiguous(), expected.detach().cpu().contiguous()
    if torch.equal(a.view(idt), e.view(idt)):
        return
    cols = a.shape[-1] if a.dim() else 1
    bad = (a.view(idt) != e.view(idt)).reshape(-1)
    i = int(bad.to(torch.uint8).argmax())
    av, ev = float(a.reshape(-1)[i]), float(e.reshape(-1)[i])
    raise AssertionError(f"{what + ': ' if what else ''}{int(bad.sum())} of {bad.numel()} elements differ; first at (row {i // cols}, column {i % cols}): "
                         f"expected {ev!r}, got {av!r}, difference {av - ev!r}")


# ---- attention held to selection / uniform / power-of-two softmaxes (tests/attn_exact_cases.py, test_gpu_exact_attention.py) ----
_MANT_MINEXP = {torch.bfloat16: (7, -126), torch.float16: (10, -14), torch.float32: (23, -126)}


def ulp_of(t64, dtype):
    """fp64 tensor -> the spacing of ``dtype`` at each value (at zero and in the subnormal range: the subnormal spacing)"""
    mant, emin = _MANT_MINEXP[dtype]
    e = torch.frexp(t64.abs().double())[1].double() - 1.0  # |t| in [2^e, 2^(e+1)); frexp(0) gives e = -1, clamped below
    e = torch.where(t64 == 0, torch.full_like(e, float(emin)), e).clamp_min(float(emin))
    return torch.exp2(e - mant)


def assert_within_half_ulp(out, ref64, absref64, dtype, what="", coeff=8.0):
    """|out - ref64| <= 0.5 ulp_dtype(ref64) + coeff * 2^-24 * absref64 (coeff 8: a result whose only inexact steps are a reciprocal, the multiply by
    it (a few fp32 ulp of the magnitude ``absref64`` = the same attention applied to |V|) and the final rounding to ``dtype``; coeff 16: a normalisation,
    tests/norm_exact_cases.py).
    The message names the first offending (row, column) of the [-1, last dim] view."""
    assert out.dtype == dtype and tuple(out.shape) == tuple(ref64.shape) == tuple(absref64.shape), \
        (what, out.dtype, dtype, tuple(out.shape), tuple(ref64.shape), tuple(absref64.shape))
    a = out.detach().cpu().double()
    ulp = ulp_of(ref64, dtype)
    err = (a - ref64).abs()
    bad = ~(err <= 0.5 * ulp + coeff * 2.0 ** -24 * absref64)  # (a NaN is bad)
    if not bool(bad.any()):
        return
    cols = a.shape[-1] if a.dim() else 1
    i = int(bad.reshape(-1).to(torch.uint8).argmax())
    av, ev, uv = float(a.reshape(-1)[i]), float(ref64.reshape(-1)[i]), float(ulp.reshape(-1)[i])
    raise AssertionError(f"{what + ': ' if what else ''}{int(bad.sum())} of {bad.numel()} elements leave the half-ulp bound; first at (row {i // cols}, "
                         f"column {i % cols}): expected {ev!r}, got {av!r}, error {(av - ev) / uv:.3f} ulp")


def nan_padded_vt(v, Lpad, dtype, device, poison=True, zero_to=None):
    """v [Bk, L, heads, d] (CPU) -> V^T [Bk, heads, d, Lpad] on ``device``; the pad columns [L, Lpad) are NaN (NAN_WORD) with ``poison``,
    else the zeros the kernels of ops.attention's layout document that they need (csrc/attention.hip: "with zero padding"); zero_to: the
    columns [L, zero_to) are zeros and only [zero_to, Lpad) NaN"""
    Bk, L, heads, d = v.shape
    assert Lpad >= L and Lpad % 32 == 0
    n = Bk * heads * d * Lpad
    buf = nan_buffer(n, dtype, device) if poison else torch.zeros(n, dtype=dtype, device=device)
    buf = buf.view(Bk, heads, d, Lpad)
    if zero_to is not None:
        buf[..., L:zero_to] = 0
    buf[..., :L] = v.permute(0, 2, 3, 1).to(device, dtype)
    return buf


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


def nan_surrounded(x, device, guard=1024):
    """the 1-D fp32 clip ``x`` (CPU tensor or array) as a view into one flat buffer [guard | len(x) | guard] whose other elements are NaN
    (NAN_WORD): a kernel that reads a sample before the clip's first or after its last gives NaN"""
    x = torch.as_tensor(x, dtype=torch.float32)
    buf = nan_buffer(x.numel() + 2 * guard, torch.float32, device)
    view = buf[guard:guard + x.numel()]
    view.copy_(x)
    return view


def nan_neighbours(x, device, before=131, after=257):
    """[all-NaN clip, x, all-NaN clip] as 1-D fp32 GPU tensors: the ragged batch whose packed buffer puts NaN on either side of ``x``"""
    return [nan_buffer(before, torch.float32, device), torch.as_tensor(x, dtype=torch.float32).to(device), nan_buffer(after, torch.float32, device)]
