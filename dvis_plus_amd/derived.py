"""Tensors derived from weights (folded FrozenBN, packed / transformed / concatenated forms): ONE staleness and refresh policy.

Stale = the fingerprint of the source tensors changed.  Refresh = the new value is copied INTO the old tensors wherever
device, dtype, shape and strides agree, because captured hipGraphs hold raw pointers to them; otherwise the new object replaces
the old.  The extra allocation and copy happen only when a weight changes, never on a hit.  A derived tensor is therefore
always an OWN tensor, never a view of a source: a refresh through a view would write to the parameter (and bump its version).
"""
import collections
import threading

import torch


def fingerprint(sources, extra=()):
    """Staleness key of `sources` (tensors or None) + hashable `extra`.  `data_ptr` and `shape` next to the version counter:
    ``p.data = other`` swaps the storage without bumping ``p._version``."""
    return tuple(None if t is None else (t._version, t.data_ptr(), t.device, t.shape) for t in sources) + tuple(extra)


def _refresh(old, new):
    if isinstance(new, tuple):
        if isinstance(old, tuple) and len(old) == len(new):
            return tuple(_refresh(o, n) for o, n in zip(old, new))
        return new
    if (torch.is_tensor(new) and torch.is_tensor(old) and old.device == new.device and old.dtype == new.dtype
            and old.shape == new.shape and old.stride() == new.stride()):
        return old.copy_(new)
    return new


class Derived:
    """One derived value of one owner (a module attribute)."""

    def __init__(self):
        self.key = self.value = None

    def get(self, sources, make, extra=()):
        """`make()` -> a tensor, or a (nested) tuple of tensors, Python scalars and Nones."""
        key = fingerprint(sources, extra)
        if key != self.key:
            self.value = _refresh(self.value, make())
            self.key = key
        return self.value


class Table:
    """Derived values of objects the caller only holds (function-level packs): one `Derived` per (id(key_obj), kind) — the same
    weight packed two ways keeps both — with least-recently-used eviction past `cap` entries (a cleared-at-once dict re-packed
    every layer of every forward once a process held more than `cap` weights; a split-f16 pack reads max|w| back to the host)."""

    def __init__(self, cap=4096):
        self.cap, self.d, self.lock = cap, collections.OrderedDict(), threading.Lock()

    def entry(self, key_obj, kind, sources, make, extra=(), note=None):
        """The refreshed entry: `.value`, and `.note` = `note()` of the call that created the entry (it survives re-makes)."""
        k = (id(key_obj), kind)
        with self.lock:                # (callers on several host threads may pack: the LRU order is shared state)
            ent = self.d.get(k)
            if ent is None:
                ent = self.d[k] = Derived()
                ent.key_obj, ent.note = key_obj, None if note is None else note()      # (holds key_obj: id() stays unique)
                while len(self.d) > self.cap:
                    self.d.popitem(last=False)
            else:
                self.d.move_to_end(k)
            ent.get(sources, make, extra)
        return ent

    def get(self, key_obj, kind, sources, make, extra=()):
        return self.entry(key_obj, kind, sources, make, extra).value

    def __len__(self):
        return len(self.d)


TABLE = Table()
