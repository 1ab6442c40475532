"""Host-side base of every module that caches a packed device copy of its weights (the plan of ``include/cookietts_hip.h``).

``PackedModule`` owns the two caches and the one rule that says when they are stale:

* ``self._packed``: whatever ``build()`` returned for ``packed(device, build)`` (a blob; a blob and its 16-bit twin; a blob and the
  conditioning operators), kept with the device and ``param_key(self)`` it was built from.  It is served again only while both
  still match.  The key catches optimizer steps and in-place updates (version counter) and tensors swapped by ``.to()`` /
  ``.half()`` (data pointer, dtype).
* ``self._ws``: the workspace of the ONE geometry that ran last (``workspace(key, size_query)``).
* ``_invalidate()`` drops both.  It runs from ``_apply`` (``.to()``, ``.half()``, ``.cuda()``), from ``load_state_dict`` and from a
  load-state-dict post hook: ``nn.Module.load_state_dict`` on a PARENT recurses through ``_load_from_state_dict`` and never calls a
  child's ``load_state_dict`` override, so an override alone would keep serving the old blob (silently wrong audio).  A subclass
  with more to drop (``W_inverse`` on the mixing modules, the decoder's exchange buffers) extends it.
* ``repack()`` is the public spelling, for the one change nothing above sees: a write through ``param.data``, which bypasses the
  version counter.
"""
from __future__ import annotations

import itertools

import torch
import torch.nn as nn

from . import _lib


def param_key(module):
    return tuple((t.data_ptr(), t._version, t.dtype) for t in itertools.chain(module.parameters(), module.buffers()))


def dev(t, keep):
    """Address of ``t`` as contiguous fp32 for a weights struct; the tensor is parked in ``keep`` until the pack call has run."""
    t = t.detach().float().contiguous()
    keep.append(t)
    return t.data_ptr()


def _drop_on_load(module, incompatible_keys):
    module._invalidate()


class PackedModule(nn.Module):
    GPU_ONLY = "HIP path needs the model on a GPU (no CPU fallback)"      # a subclass names itself in front of this

    def __init__(self):
        super().__init__()
        self._packed = None      # (device, param key, what build() returned)
        self._ws = {}            # key of the live geometry (device first) -> its workspace
        self.register_load_state_dict_post_hook(_drop_on_load)

    def _invalidate(self):
        self._packed, self._ws = None, {}

    def _apply(self, fn, *a, **kw):
        self._invalidate()
        return super()._apply(fn, *a, **kw)

    def load_state_dict(self, state_dict, strict=True, **kw):
        self._invalidate()
        return super().load_state_dict(state_dict, strict=strict, **kw)

    def repack(self):
        """Call after modifying parameters through ``.data``; the next call re-ingests the weights."""
        self._invalidate()

    def packed(self, device, build):
        """The packed form of the current parameters on ``device``: the cached one while nothing changed, else ``build()``."""
        key = param_key(self)
        p = self._packed
        if p is not None and p[0] == device and p[1] == key:
            return p[2]
        if p is not None:
            self._invalidate()
        if device.type != 'cuda':
            raise _lib.HipLibraryError(self.GPU_ONLY)
        value = build()
        self._packed = (device, key, value)
        return value

    def _drop_workspaces(self):
        self._ws = {}

    def workspace(self, key, size_query, zero=True):
        """The fp32 workspace of geometry ``key`` (``key[0]`` is its device); one geometry is live at a time.  ``size_query()``
        gives its bytes - or a list of byte counts for a list of buffers - and raises for a geometry the library refuses, which
        leaves the live one alone."""
        ws = self._ws.get(key)
        if ws is None:
            sizes = size_query()
            self._drop_workspaces()
            alloc = torch.zeros if zero else torch.empty
            if isinstance(sizes, list):
                ws = [alloc(n // 4, dtype=torch.float32, device=key[0]) for n in sizes]
            else:
                ws = alloc(sizes // 4, dtype=torch.float32, device=key[0])
            self._ws[key] = ws
        return ws
