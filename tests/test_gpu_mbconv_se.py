"""The tiny EfficientNet-B0 and MobileNetV3-Large models of models/mbconv_se.py through the HIP engine, with the
SE blocks on the se kernel (kernels/se.hip) and unfused (EngineOptions::fuse_se = false), against torch_forward
on the GPU under the project's model bars (fp32 rel-L2 <= 1e-4 with identical top-1, bf16 rel-L2 <= 2e-2), and
one EfficientNet-B0 224 x 224 run in fp32."""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

BATCHES = (1, 5)


@pytest.fixture(scope="module", params=["efficientnet_b0", "mobilenet_v3_large"])
def tiny(request, native, tmp_path_factory):
    """(name, path, {B: (x, torch fp32 output)}): the references are computed once per model"""
    import torch

    from die_amd.models import mbconv_se as ms

    cfg = ms.tiny_config(request.param)
    blob, w = ms.build_onnx(cfg)
    path = str(tmp_path_factory.mktemp("se_" + request.param) / "model.onnx")
    open(path, "wb").write(blob)
    refs = {}
    for B in BATCHES:
        x = ms.synthetic_input(B, cfg, seed=40 + B)
        with torch.no_grad():
            refs[B] = (x, ms.torch_forward(w, x, cfg, device="cuda").double().cpu().numpy())
    return request.param, path, refs


@pytest.mark.parametrize("fuse_se", [True, False])
@pytest.mark.parametrize("precision,tol", [("fp32", 1e-4), ("bf16", 2e-2)])
def test_tiny_models_match_torch(native, tiny, precision, tol, fuse_se):
    name, path, refs = tiny
    eng = native.Engine(path, device="hip", max_batch=8, precision=precision, autotune=False, fuse_se=fuse_se)
    try:
        info = eng.refresh_info()
        assert info["name"].startswith("hip:gfx950") and info["options"]["fuse_se"] is fuse_se
        for B in BATCHES:
            x, ref = refs[B]
            got = eng.run(x.reshape(B, -1)).astype(np.float64)
            err = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
            print("%s tiny %s fuse_se=%s B=%d rel-L2 vs torch %.2e" % (name, precision, fuse_se, B, err))
            assert got.shape == ref.shape and err <= tol, (name, precision, fuse_se, B, err)
            if precision == "fp32":
                assert (got.argmax(1) == ref.argmax(1)).all(), (name, B)
    finally:
        eng.close()


def test_b0_224_matches_torch(native, tmp_path):
    import torch

    from die_amd.models import mbconv_se as ms

    cfg = ms.MbconvSeConfig("efficientnet_b0")
    blob, w = ms.build_onnx(cfg)
    path = str(tmp_path / "b0_224.onnx")
    open(path, "wb").write(blob)
    x = ms.synthetic_input(2, cfg, seed=3)
    with torch.no_grad():
        ref = ms.torch_forward(w, x, cfg, device="cuda").double().cpu().numpy()
    eng = native.Engine(path, device="hip", max_batch=2, precision="fp32", autotune=False)
    try:
        got = eng.run(x.reshape(2, -1)).astype(np.float64)
    finally:
        eng.close()
    err = float(np.linalg.norm(got - ref) / np.linalg.norm(ref))
    print("efficientnet-b0 224 fp32 B=2 rel-L2 vs torch %.2e" % err)
    assert err <= 1e-4 and (got.argmax(1) == ref.argmax(1)).all(), err
