"""Cases shared by tests/test_exchange_cut.py (CPU) and tests/test_exchange_gpu.py: where the tape runs the early-exchange hook
in each model (backbones/functional.py) and the frozen sets both files go through."""

MODELS = ("utae", "timeunet", "wtae")

# Top-level blocks whose gradients are NOT written yet when the backward pass reaches the hook: the blocks that the forward
# runs before `ctx.tape.record(ctx.early_hook)`.  Everything else has been written by then.
UNWRITTEN = {"utae": ("in_conv.", "down_blocks."), "timeunet": ("in_conv.",), "wtae": ("in_conv.", "spatial_reduction.")}
# The block that follows them in named_parameters(): the early bucket starts at its first parameter.
FIRST_EARLY = {"utae": "up_blocks.", "timeunet": "down_blocks.", "wtae": "down_blocks."}

PATTERNS = ("all", "encoder", "te", "head+up0", "alternate")


def model_class(model):
    import crop2seg_amd as C2S
    return {"utae": C2S.UTAE, "timeunet": C2S.TimeUNet_v1, "wtae": C2S.WTAE}[model]


def flags_for(model, names, pattern):
    """requires_grad of every parameter under a pattern: "all" trains everything; "encoder" freezes the prefix the hook has
    not reached; "te" freezes the temporal encoder, a hole inside the suffix; "head+up0" freezes the head and the first
    decoder block; "alternate" freezes every second parameter."""
    if pattern == "all":
        return [True] * len(names)
    if pattern == "alternate":
        return [i % 2 == 0 for i in range(len(names))]
    frozen = {"encoder": UNWRITTEN[model], "te": ("temporal_encoder.",), "head+up0": ("out_conv.", "up_blocks.0.")}[pattern]
    flags = [not n.startswith(frozen) for n in names]
    assert not all(flags) and any(flags)
    return flags


def written_at_hook(model, names, flags):
    """Names in ctx._gwritten when the hook runs: the trainable parameters of the blocks behind the hook."""
    return {n for n, f in zip(names, flags) if f and not n.startswith(UNWRITTEN[model])}
