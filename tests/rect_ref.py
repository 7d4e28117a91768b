"""Shared pieces of the rectangle tests (test_models_rect.py, test_models_rect_gpu.py): the seeded models and the stand-in for
the oracle's att_group aggregator on wide inputs (CPU only).

The reference's TemporalAggregator tests `x.shape[-2] > w` (temporal_aggregator.py:26): the map's HEIGHT against the
attention's WIDTH.  On a U-TAE input with W >= 2H the coarsest skip map is no higher than the attention is wide (16 x 64:
the 4 x 16 map against the 2 x 8 attention), the avg_pool2d branch is taken with a kernel of 2 or more and the following view
raises; oracle.crop2seg_oracle.temporal_aggregate restates that faithfully and raises too.  This project up-samples
bilinearly whenever the map is larger than the attention, which is what `aggregate_bilinear_either`
evaluates: the oracle's function with the comparison made in both directions.  Where the reference is defined (H > w on every
skip map) the two are the same code path: tests/test_models_rect.py holds them bit for bit."""
import torch
import torch.nn.functional as F

from oracle.crop2seg_oracle import temporal_aggregate as ORACLE_AGGREGATE      # the unwrapped one, whatever a test patches in

MODELS = ("utae", "timeunet", "wtae")


def aggregate_bilinear_either(x, pad_mask, attn, mode="att_group"):
    """oracle.crop2seg_oracle.temporal_aggregate, with the bilinear branch whenever the map is larger than the attention in
    either direction (the oracle: when H > w)."""
    if mode != "att_group":
        return ORACLE_AGGREGATE(x, pad_mask, attn, mode)
    B, T, C, H, W = x.shape
    nh, _, _, h, w = attn.shape
    a = attn.reshape(nh * B, T, h, w)
    if H > h or W > w:
        a = F.interpolate(a, size=(H, W), mode="bilinear", align_corners=False)
    else:
        a = F.avg_pool2d(a, kernel_size=w // H)
    a = a.view(nh, B, T, H, W)
    if pad_mask is not None and bool(pad_mask.any()):
        a = a * (~pad_mask).to(a.dtype)[None, :, :, None, None]
    xs = x.view(B, T, nh, C // nh, H, W)
    return torch.einsum("nbthw,btnchw->bnchw", a, xs).reshape(B, C, H, W)


def outside_reference_domain(model, H, W):
    """U-TAE with att_group on W >= 2H: the reference's aggregator raises (see the module docstring)."""
    return model == "utae" and W >= 2 * H


def net(model, sd=None, **ctor):
    import crop2seg_amd as C2S
    cls = {"utae": C2S.UTAE, "timeunet": C2S.TimeUNet_v1, "wtae": C2S.WTAE}[model]
    n = cls(**{**dict(input_dim=10, out_conv=[32, 15]), **ctor})
    if sd is not None:
        n.load_state_dict(sd)
    return n


def state(model, seed=41, **ctor):
    from oracle import seeded
    ks = [(k, tuple(v.shape)) for k, v in net(model, **ctor).state_dict().items()]
    return seeded.make_state(ks, seed, "tame")
