from . import _lib  # (reads CRG_BATCH_INVARIANT at import; loads nothing)


def set_ff_precision(module, precision):
    """Set the precision of every FeedForward below `module` (UNet, ControlNet, SDXL base / refiner, or any part of them): "mx8" = both
    feed-forward GEMMs on block-scaled e4m3 operands (ops.linear_mx8; half-type activations only), None = the default path.  Returns
    the number of modules switched.  Captured graphs of the model are re-captured on their next call."""
    from .ldm_hip.transformer import FeedForward
    from .ops import TensorKeyedCache
    if precision not in (None, "mx8"):
        raise ValueError(f"set_ff_precision: precision {precision!r} (None or 'mx8')")
    n = 0
    for m in module.modules():
        if isinstance(m, FeedForward):
            m.precision = precision
            n += 1
    TensorKeyedCache.generation += 1  # part of GraphedModule's stamp: a graph captured under the other precision is not replayed
    return n


def set_batch_invariant(tune_samples=8):
    """Batch-invariant mode (include/crg_hip.h, crg_ctx_set_invariant): with it on, what the library computes for one
    sample is a function of that sample, the weights and `tune_samples` only - bit-identical alone, at any position of any batch and
    on any rank of a sharded run.  Every size heuristic (kernel family, tile configuration, K slices, GroupNorm chunking, attention
    kernel, ...) then reads `tune_samples` samples of the per-sample problem instead of the call's size; 8 is the UNet batch of the
    headline workload, whose routes therefore stay what they are.  None or 0 turns the mode off (the default: nothing changes).
    Sets every live context and those created later; captured graphs are re-captured on their next call.  CRG_BATCH_INVARIANT=<n> in
    the environment does the same at import.  A bool, a negative number or a non-integer is a ValueError."""
    n = _lib.parse_invariant(tune_samples)
    _lib.set_invariant(n)
    from .ops import TensorKeyedCache
    TensorKeyedCache.generation += 1  # part of GraphedModule's stamp: a graph captured under other routes is not replayed
    return n


def batch_invariant():
    """tune_samples of the batch-invariant mode, or 0 while it is off."""
    return _lib.invariant()
