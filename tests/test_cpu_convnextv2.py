"""The CPU executor on ConvNeXt-V2 (tiny config, both export forms of the GRN chain) against the float64
torch oracle: ReduceL2 over the two spatial axes of a rank-4 activation, the mean over its last axis and the
[1,1,1,C] broadcasts.  The bar is the one of tests/test_cpu_convnext.py (rel-L2 < 1e-5)."""
import numpy as np
import pytest

SPECS = ["timm", "hf"]


@pytest.fixture(scope="module")
def v2_models(native, tmp_path_factory):
    from die_amd.models import convnextv2 as v2

    d = tmp_path_factory.mktemp("convnextv2_cpu")
    out = {}
    for spec in SPECS:
        cfg = v2.tiny_convnextv2_config(**v2.SPECS[spec])
        blob, w = v2.build_onnx(cfg)
        p = str(d / (spec + ".onnx"))
        open(p, "wb").write(blob)
        out[spec] = (p, w, cfg)
    return out


@pytest.mark.parametrize("spec", SPECS)
@pytest.mark.parametrize("B", [1, 3])
def test_cpu_executor_matches_torch(native, v2_models, spec, B):
    import torch

    from die_amd.models import convnextv2 as v2

    path, w, cfg = v2_models[spec]
    x = v2.synthetic_input(B, cfg, seed=10 + B)
    got = native.cpu_run(path, x)
    with torch.no_grad():
        ref = v2.torch_forward(w, x, cfg, dtype=torch.float64).numpy()
    assert got.shape == (B, cfg.num_classes) and np.isfinite(got).all()
    err = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    assert err < 1e-5, (spec, B, err)
    assert (got.argmax(1) == ref.argmax(1)).all()


def test_export_forms_are_one_network(native, v2_models):
    """the two graphs compute the same function of the same weights"""
    from die_amd.models import convnextv2 as v2

    cfg = v2_models["timm"][2]
    x = v2.synthetic_input(2, cfg, seed=3)
    a, b = (native.cpu_run(v2_models[s][0], x) for s in SPECS)
    assert float(np.linalg.norm(b - a) / np.linalg.norm(a)) < 1e-5
    for k, v in v2_models["timm"][1].items():
        assert np.array_equal(v, v2_models["hf"][1][k]), k


def test_grn_matters_in_the_output():
    """with the checkpoints' init of zeros GRN is the identity and a bug in it would hide below every
    tolerance: the generator's init must not"""
    import torch

    from die_amd.models import convnextv2 as v2

    cfg = v2.tiny_convnextv2_config()
    w = v2.make_weights(cfg)
    x = v2.synthetic_input(2, cfg)
    w0 = dict(w)
    for k in w:
        if k.endswith("grn.weight") or k.endswith("grn.bias"):
            w0[k] = np.zeros_like(w[k])
    with torch.no_grad():
        a = v2.torch_forward(w, x, cfg).numpy()
        b = v2.torch_forward(w0, x, cfg).numpy()
    assert np.linalg.norm(a - b) / np.linalg.norm(a) > 0.1


def test_configs():
    from die_amd.models import convnextv2 as v2

    cfg = v2.ConvNeXtV2Config()
    assert (cfg.depths, cfg.dims, cfg.image, cfg.num_classes, cfg.grn_eps) == ((3, 3, 9, 3), (96, 192, 384, 768), 224, 1000, 1e-6)
    w = v2.make_weights(cfg)
    assert sum(v.size for v in w.values()) == 28635496  # ConvNeXt-V2-T's parameter count
    a = v2.atto_config()
    assert (a.depths, a.dims, a.image) == ((2, 2, 6, 2), (40, 80, 160, 320), 224)
    t = v2.tiny_convnextv2_config()
    assert (t.depths, t.dims, t.image) == ((1, 1, 2, 1), (16, 32, 64, 128), 32)
