"""RegNet X / Y through the HIP engine: tiny_regnet_config() (grouped 3x3 convs of width 24, 40, 48, 56, 64 on 72,
120, 96, 168, 128 channels, three of them stride 2; Y adds the SE blocks) against torch_forward on the GPU in fp32
and the fp32 CPU executor, under the bars of tests/test_gpu_resnext.py: fp32 rel-L2 <= 1e-4 with identical top-1,
bf16 rel-L2 <= 2e-2.  With EngineOptions::mfma_gconv off the grouped convs run on gconv_kernel with fp32 weights:
the same bars, not the same bits."""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

BATCHES = (1, 5)


@pytest.fixture(scope="module", params=[False, True], ids=["x", "y"])
def rn_model(native, tmp_path_factory, request):
    """(path, {B: (x, torch fp32 logits, cpu executor logits)}): the references are computed once"""
    import torch

    from die_amd.models import regnet as rn

    cfg = rn.tiny_regnet_config(se=request.param)
    blob, w = rn.build_onnx(cfg)
    path = str(tmp_path_factory.mktemp("regnet_gpu") / "regnet_tiny.onnx")
    open(path, "wb").write(blob)
    refs = {}
    for B in BATCHES:
        x = rn.synthetic_input(B, cfg, seed=30 + B)
        with torch.no_grad():
            t = rn.torch_forward(w, x, cfg, device="cuda").double().cpu().numpy()
        refs[B] = (x, t, native.cpu_run(path, x).reshape(B, -1))
    return path, refs


@pytest.mark.parametrize("mfma", [True, False])
@pytest.mark.parametrize("precision,tol", [("fp32", 1e-4), ("bf16", 2e-2)])
def test_tiny_regnet_matches_torch_and_cpu_executor(native, rn_model, precision, tol, mfma):
    path, refs = rn_model
    eng = native.Engine(path, device="hip", max_batch=8, precision=precision, autotune=False, mfma_gconv=mfma)
    try:
        info = eng.refresh_info()
        assert info["name"].startswith("hip:gfx950"), info["name"]
        assert info["options"]["mfma_gconv"] is mfma
        for B in BATCHES:
            x, tref, cpu = refs[B]
            got = eng.run(x.reshape(B, -1)).astype(np.float64)
            assert got.shape == tref.shape and np.isfinite(got).all()
            e_t = float(np.linalg.norm(got - tref) / np.linalg.norm(tref))
            e_cpu = float(np.linalg.norm(got - cpu) / np.linalg.norm(cpu))
            print("regnet tiny %s mfma=%s B=%d rel-L2 vs torch %.2e vs cpu %.2e" % (precision, mfma, B, e_t, e_cpu))
            assert e_t <= tol, (precision, mfma, B, e_t)
            if precision == "fp32":
                assert e_cpu <= 1e-4, (mfma, B, e_cpu)
                assert (got.argmax(1) == tref.argmax(1)).all(), (mfma, B)
    finally:
        eng.close()
