"""Which copy of an int4 (W4A16) layer's weights is resident, and the packed copies derived from its parameters, each
kept under its sources' ``(data_ptr, _version)``.  A write through ``param.data`` moves no version: :func:`drop_derived`."""

from __future__ import annotations

import torch

_ON_TENSOR = "_ll_prepacked"  # (key, (packed weight, packed scales)) of the reference-signature route, on its ``qweight``


def keyed(obj, key, build, name: str = _ON_TENSOR):
    """``obj.<name>`` if it was built for ``key``; else -- outside a graph capture -- ``build()``, kept there under ``key``.
    ``None``: nothing valid is cached and nothing may be built now (a capture, or ``build`` returned None).  ``name``: a
    record's ``weight`` / ``scales``, or the pair kernels/quantization.py::_auto_prepacked keeps on a ``qweight``."""
    hit = getattr(obj, name, None)
    if hit is not None and hit[0] == key:
        return hit[1]
    value = None if torch.cuda.is_current_stream_capturing() else build()
    if value is not None:
        setattr(obj, name, (key, value))
    return value


class W4Layouts:
    """The record on a W4A16 layer or merged q|k|v / gate|up holder.  ``weight`` / ``scales``: ``(key, copy)`` of
    ``pack_w4a16_weights`` / ``pack_w4a16_scales`` (:func:`keyed`).  ``compact``: ``layer.weight`` aliases the packed layout.
    ``member``: ``(holder, rows)`` -- ``layer.weight`` views those rows of a compacted holder's packed words."""

    weight = scales = member = None
    compact = False

    @staticmethod
    def of(obj, create: bool = True) -> W4Layouts | None:
        rec = getattr(obj, "_w4_layouts", None)
        if rec is None and create:
            rec = W4Layouts()
            setattr(obj, "_w4_layouts", rec)
        return rec


def holds_packed(obj) -> bool:
    """Whether ``obj.weight`` holds packed words rather than reference rows: compacted, or a member of a compacted holder."""
    rec = W4Layouts.of(obj, create=False)
    return rec is not None and (rec.compact or rec.member is not None)


def drop_derived(obj) -> None:
    """The one invalidation path: forget the packed copies of a layer, holder or weight tensor (not the compact state)."""
    rec = W4Layouts.of(obj, create=False)
    if rec is not None:
        rec.weight = rec.scales = None
    if isinstance(obj, torch.Tensor) and hasattr(obj, _ON_TENSOR):
        delattr(obj, _ON_TENSOR)


def derived_tensors(obj) -> list:
    """The packed copies ``obj`` keeps resident."""
    rec = W4Layouts.of(obj, create=False)
    return [] if rec is None else [c[1] for c in (rec.weight, rec.scales) if c is not None]
