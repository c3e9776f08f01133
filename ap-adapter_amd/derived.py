"""Derived weights: copies of parameters re-laid-out, packed, transposed, stacked or folded so that a kernel can read them.

Every one of them is cached here, on the parameter it derives from.  An entry lives as long as that parameter (the store is weakly
keyed by its identity) and is replaced -- its old value released -- when the signature of the parameter, of the other tensors it was
built from or of the settings it was built with changes.  Nothing else drops a value: a captured hipGraph holds the raw addresses of
the derived weights it was recorded with, and the pipeline re-captures whenever a parameter changes (pipeline._weights_signature).
"""
import torch
from torch.utils.weak import WeakIdKeyDictionary

_store = WeakIdKeyDictionary()  # key tensor -> {tag: (signature, value)}
_values = WeakIdKeyDictionary()  # every tensor a make() returned (alone or in a tuple / list) -> True


def signature(*tensors):
    """what "this parameter changed" means: a tensor re-assigned, moved, cast, reshaped or updated in place (None for None)"""
    return tuple(None if t is None else (id(t), t.data_ptr(), t._version, t.dtype, t.device, t.shape) for t in tensors)


def derived(key, tag, make, deps=(), extra=()):
    """``make()``'s value for (key, tag), built once and rebuilt when ``signature(key, *deps) + extra`` changes.

    ``key`` is the tensor the module holds, never a fresh view (a view would never hit).  ``make`` reads nothing besides ``key``,
    ``deps`` and ``extra``, and its value must not reference ``key`` (build it from ``key.detach()``), or the entry keeps its key alive."""
    sig = signature(key, *deps) + tuple(extra)
    entries = _store.setdefault(key, {})
    hit = entries.get(tag)
    if hit is None or hit[0] != sig:
        value = make()
        for t in (value if isinstance(value, (tuple, list)) else (value,)):
            if isinstance(t, torch.Tensor):
                _values[t] = True
        hit = entries[tag] = (sig, value)
    return hit[1]


def is_derived(t):
    """True when ``t`` is a value this store built: a tensor nothing writes into after make(), replaced (as a new tensor) when what it
    derives from changes"""
    return t in _values
