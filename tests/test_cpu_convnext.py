"""The CPU executor on ConvNeXt (tiny config, every export form) against the float64 torch oracle: the 4-D
Transposes in both directions, MatMul of a rank-4 activation with a 2-D weight, LayerNormalization on rank
4, ReduceMean(axes [1]) on NCHW and the [C,1,1] broadcasts of the channels-first LayerNorm.  The bar is the
one tests/test_op_coverage.py holds generated models to against torch (rel-L2 < 1e-5)."""
import numpy as np
import pytest

SPECS = ["timm", "channels_first_ln", "reduce_mean_head"]


@pytest.fixture(scope="module")
def cn_models(native, tmp_path_factory):
    from die_amd.models import convnext as cn

    d = tmp_path_factory.mktemp("convnext_cpu")
    out = {}
    for spec in SPECS:
        cfg = cn.tiny_convnext_config(**cn.SPECS[spec])
        blob, w = cn.build_onnx(cfg)
        p = str(d / (spec + ".onnx"))
        open(p, "wb").write(blob)
        out[spec] = (p, w, cfg)
    return out


@pytest.mark.parametrize("spec", SPECS)
@pytest.mark.parametrize("B", [1, 3])
def test_cpu_executor_matches_torch(native, cn_models, spec, B):
    import torch

    from die_amd.models import convnext as cn

    path, w, cfg = cn_models[spec]
    x = cn.synthetic_input(B, cfg, seed=10 + B)
    got = native.cpu_run(path, x)
    with torch.no_grad():
        ref = cn.torch_forward(w, x, cfg, dtype=torch.float64).numpy()
    assert got.shape == (B, cfg.num_classes) and np.isfinite(got).all()
    err = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    assert err < 1e-5, (spec, B, err)
    assert (got.argmax(1) == ref.argmax(1)).all()


def test_export_forms_are_one_network(native, cn_models):
    """the three graphs compute the same function of the same weights"""
    from die_amd.models import convnext as cn

    cfg = cn_models["timm"][2]
    x = cn.synthetic_input(2, cfg, seed=3)
    ys = [native.cpu_run(cn_models[s][0], x) for s in SPECS]
    for y in ys[1:]:
        assert float(np.linalg.norm(y - ys[0]) / np.linalg.norm(ys[0])) < 1e-5


def test_layer_scale_matters_in_the_output():
    """with timm's 1e-6 init an MLP bug would hide below every tolerance: the default init must not"""
    import torch

    from die_amd.models import convnext as cn

    cfg = cn.tiny_convnext_config()
    w = cn.make_weights(cfg)
    x = cn.synthetic_input(2, cfg)
    w0 = dict(w)
    for k in w:
        if k.endswith("gamma"):
            w0[k] = np.zeros_like(w[k])
    with torch.no_grad():
        a = cn.torch_forward(w, x, cfg).numpy()
        b = cn.torch_forward(w0, x, cfg).numpy()
    assert np.linalg.norm(a - b) / np.linalg.norm(a) > 0.1


def test_default_config_is_convnext_t():
    from die_amd.models import convnext as cn

    cfg = cn.ConvNeXtConfig()
    assert (cfg.depths, cfg.dims, cfg.image, cfg.num_classes, cfg.eps) == ((3, 3, 9, 3), (96, 192, 384, 768), 224, 1000, 1e-6)
    assert cn.synthetic_input(1, cfg).size == 150528
    w = cn.make_weights(cfg)
    assert sum(v.size for v in w.values()) == 28589128  # ConvNeXt-T's parameter count
