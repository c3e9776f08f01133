"""CPU: the derived-weight cache (ap_adapter_amd.derived) -- when an entry is rebuilt, and that it dies with its key."""
import gc
import weakref

import torch

from ap_adapter_amd import autograd as AG
from ap_adapter_amd.derived import derived, signature
from ap_adapter_amd.unet import Conv3x3


class _Counter:
    """a make() that counts its calls and returns a fresh tensor each time"""

    def __init__(self, fn):
        self.fn, self.calls = fn, 0

    def __call__(self):
        self.calls += 1
        return self.fn()


def test_hit_returns_the_same_object_and_builds_once():
    w = torch.randn(8, 4)
    make = _Counter(lambda: w.detach().t().contiguous())
    a = derived(w, "t", make)
    assert derived(w, "t", make) is a and make.calls == 1
    assert torch.equal(a, w.t())


def test_in_place_update_rebuilds():
    w = torch.nn.Parameter(torch.randn(8, 4))
    make = _Counter(lambda: w.detach() * 2)
    a = derived(w, "x2", make)
    with torch.no_grad():
        w.mul_(3)
    b = derived(w, "x2", make)
    assert b is not a and make.calls == 2 and torch.equal(b, w.detach() * 2)


def test_reassigned_dep_rebuilds():
    lin = torch.nn.Linear(4, 8)
    make = _Counter(lambda: lin.weight.detach() + lin.bias.detach()[:, None])
    a = derived(lin.weight, "wb", make, (lin.bias,))
    assert derived(lin.weight, "wb", make, (lin.bias,)) is a
    lin.bias = torch.nn.Parameter(torch.ones(8))
    b = derived(lin.weight, "wb", make, (lin.bias,))
    assert b is not a and make.calls == 2 and torch.equal(b, lin.weight.detach() + 1)


def test_dtype_cast_rebuilds():
    lin = torch.nn.Linear(4, 8, bias=False)
    make = _Counter(lambda: lin.weight.detach().clone())
    a = derived(lin.weight, "copy", make)
    lin.to(torch.float64)  # (a cast keeps the Parameter object and swaps its data)
    b = derived(lin.weight, "copy", make)
    assert b is not a and make.calls == 2 and b.dtype == torch.float64


def test_changed_extra_rebuilds_and_releases_the_previous_value():
    w = torch.randn(8, 4)
    a = derived(w, "pad", lambda: torch.cat([w, w.new_zeros(1, 4)]), extra=(1,))
    ra = weakref.ref(a)
    del a
    b = derived(w, "pad", lambda: torch.cat([w, w.new_zeros(2, 4)]), extra=(2,))
    gc.collect()
    assert b.shape == (10, 4) and ra() is None
    assert derived(w, "pad", lambda: None, extra=(2,)) is b


def test_two_tags_on_one_key_coexist():
    w = torch.randn(8, 4)
    a = derived(w, "a", lambda: w.detach() + 1)
    b = derived(w, "b", lambda: w.detach() + 2)
    assert derived(w, "a", lambda: None) is a and derived(w, "b", lambda: None) is b


def test_value_dies_with_its_key():
    w = torch.randn(64, 64)
    r = weakref.ref(derived(w, "t", lambda: w.detach().t().contiguous()))
    gc.collect()
    assert r() is not None
    del w
    gc.collect()
    assert r() is None


def test_signature_tracks_identity_storage_version_type_place_and_shape():
    w = torch.randn(8, 4)
    s = signature(w, None)
    assert s == signature(w, None) and s[1] is None
    assert signature(w.view(4, 8), None) != s  # another tensor object (and shape) over the same storage
    w.add_(1)
    assert signature(w, None) != s


def test_conv3x3_packed_and_autograd_wt_hit_rebuild_and_release():
    conv = Conv3x3(4, 8).requires_grad_(False)
    w = conv.conv.weight
    p = conv.packed()
    assert conv.packed() is p and AG._conv_fwd_w(w) is p  # inference and the training forward share one copy
    assert torch.equal(p, w.permute(0, 2, 3, 1).reshape(8, 36))
    with torch.no_grad():
        w.mul_(0.5)
    p2 = conv.packed()
    assert p2 is not p and torch.equal(p2, w.permute(0, 2, 3, 1).reshape(8, 36))
    lin = torch.nn.Linear(4, 8).requires_grad_(False)
    wt = AG._wt(lin.weight)
    assert AG._wt(lin.weight) is wt and torch.equal(wt, lin.weight.t())
    with torch.no_grad():
        lin.weight.mul_(2)
    assert AG._wt(lin.weight) is not wt
    refs = weakref.ref(conv.packed()), weakref.ref(AG._wt(lin.weight))
    del conv, w, p, p2, lin, wt
    gc.collect()
    assert all(r() is None for r in refs)


def test_trainable_weights_are_not_cached():
    lin = torch.nn.Linear(4, 8)
    assert AG._wt(lin.weight) is not AG._wt(lin.weight)


def test_folded_layernorm_weights_die_with_the_weight():
    from ap_adapter_amd import ops
    w, g, b = torch.randn(64, 64), torch.ones(64), torch.zeros(64)
    wg, cs, bb = ops._ln_folded(w, None, g, b)
    assert ops._ln_folded(w, None, g, b)[0] is wg
    r = weakref.ref(wg)
    del wg, cs, bb, w
    gc.collect()
    assert r() is None
