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
