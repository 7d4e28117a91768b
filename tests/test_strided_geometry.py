"""Constructor side of the stride-2 down / up convolution geometries (CPU): the supported set, the refusals, and the
state_dict layout of the new geometries against the reference's (the key lists of the golden fixtures)."""
import json
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
FIXTURES = ["utae_train_k2_tame", "utae_eval_k6_tame", "timeunet_train_k6_tame", "timeunet_eval_k2_tame",
            "wtae_train_k2_tame", "wtae_eval_k6_tame", "utae_eval_dwsep_k6_tame"]


def _cls(model):
    import crop2seg_amd as C2S
    return {"utae": C2S.UTAE, "timeunet": C2S.TimeUNet_v1, "wtae": C2S.WTAE}[model]


@pytest.mark.parametrize("name", FIXTURES)
def test_state_dict_matches_reference(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    meta = json.loads(str(z["meta"]))
    ctor = meta["ctor"]
    assert ctor["str_conv_k"] in (2, 6) and ctor["str_conv_s"] == 2
    net = _cls(meta["model"])(input_dim=10, out_conv=[32, 15], **ctor)
    got = [(k, list(v.shape)) for k, v in net.state_dict().items()]
    ref = [(str(k), json.loads(str(s))) for k, s in zip(z["keys"], z["shapes"])]
    assert got == ref


@pytest.mark.parametrize("model", ["utae", "timeunet", "wtae"])
@pytest.mark.parametrize("k,s,p", [(2, 2, 0), (6, 2, 2)])
def test_constructor_accepts(model, k, s, p):
    net = _cls(model)(input_dim=10, str_conv_k=k, str_conv_s=s, str_conv_p=p)
    assert (net.spec.str_conv_k, net.spec.str_conv_s, net.spec.str_conv_p) == (k, s, p)


@pytest.mark.parametrize("model", ["utae", "timeunet", "wtae"])
@pytest.mark.parametrize("k,s,p", [(3, 2, 1), (8, 2, 3), (2, 1, 0), (3, 1, 1), (6, 2, 1)])
def test_constructor_refuses(model, k, s, p):
    with pytest.raises(NotImplementedError) as ei:
        _cls(model)(input_dim=10, str_conv_k=k, str_conv_s=s, str_conv_p=p)
    msg = str(ei.value)
    assert "str_conv_k=4" in msg and "(2, 2, 0)" in msg and "(6, 2, 2)" in msg
