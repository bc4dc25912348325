"""EfficientNet-Lite0 and MobileNetV2 through the HIP engine with their depthwise convs on the polyphase kernel
(kernels/dwconv_poly.hip): the tiny configs against torch_forward on the GPU under the bars of the MobileNet
test in tests/test_gpu_op_coverage.py (fp32 rel-L2 <= 1e-4 with identical top-1, bf16 rel-L2 <= 2e-2), the
logits bit for bit those of EngineOptions::poly_dwconv = false (gconv_kernel), and one Lite0-224 run in fp32."""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

BATCHES = (1, 5)


def _model(which):
    from die_amd.models import efficientnet_lite as el
    from die_amd.models import mobilenet as mb

    return (el, el.tiny_efficientnet_lite_config()) if which == "lite0" else (mb, mb.tiny_mobilenet_config())


@pytest.fixture(scope="module", params=["lite0", "mobilenet"])
def tiny(request, native, tmp_path_factory):
    """(name, path, {B: (x, torch fp32 output)}): the references are computed once per model"""
    import torch

    mod, cfg = _model(request.param)
    blob, w = mod.build_onnx(cfg)
    path = str(tmp_path_factory.mktemp("poly_" + request.param) / "model.onnx")
    open(path, "wb").write(blob)
    refs = {}
    for B in BATCHES:
        x = mod.synthetic_input(B, cfg, seed=40 + B)
        with torch.no_grad():
            refs[B] = (x, mod.torch_forward(w, x, cfg, device="cuda").double().cpu().numpy())
    return request.param, path, refs


@pytest.mark.parametrize("precision,tol", [("fp32", 1e-4), ("bf16", 2e-2)])
def test_tiny_models_match_torch_and_the_gconv_path(native, tiny, precision, tol):
    name, path, refs = tiny
    outs = {}
    for poly in (True, False):
        eng = native.Engine(path, device="hip", max_batch=8, precision=precision, autotune=False, poly_dwconv=poly)
        try:
            info = eng.refresh_info()
            assert info["name"].startswith("hip:gfx950") and info["options"]["poly_dwconv"] is poly
            outs[poly] = [eng.run(refs[B][0].reshape(B, -1)) for B in BATCHES]
        finally:
            eng.close()
    for B, got, off in zip(BATCHES, outs[True], outs[False]):
        ref = refs[B][1]
        err = float(np.linalg.norm(got.astype(np.float64) - ref) / np.linalg.norm(ref))
        print("%s tiny %s B=%d rel-L2 vs torch %.2e" % (name, precision, B, err))
        assert got.shape == ref.shape and err <= tol, (name, precision, B, err)
        if precision == "fp32":
            assert (got.argmax(1) == ref.argmax(1)).all(), (name, B)
        assert np.array_equal(got.view(np.uint32), off.view(np.uint32)), (name, precision, B)


def test_lite0_224_matches_torch(native, tmp_path):
    import torch

    from die_amd.models import efficientnet_lite as el

    cfg = el.EfficientNetLiteConfig()
    blob, w = el.build_onnx(cfg)
    path = str(tmp_path / "lite0_224.onnx")
    open(path, "wb").write(blob)
    x = el.synthetic_input(2, cfg, seed=3)
    with torch.no_grad():
        ref = el.torch_forward(w, x, cfg, device="cuda").double().cpu().numpy()
    eng = native.Engine(path, device="hip", max_batch=2, precision="fp32", autotune=False)
    try:
        got = eng.run(x.reshape(2, -1)).astype(np.float64)
    finally:
        eng.close()
    err = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    print("lite0 224 fp32 B=2 rel-L2 vs torch %.2e" % err)
    assert err <= 1e-4 and (got.argmax(1) == ref.argmax(1)).all(), err
