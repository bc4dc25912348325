"""ConvNeXt through the HIP engine: the tiny config in every export form against the fp32 CPU executor and
the torch oracle (the bars tests/test_gpu_general.py holds generated models to: fp32 rel-L2 <= 1e-4 and the
same top-1, bf16 rel-L2 <= 3e-2), the tiled depthwise kernel against gconv_kernel inside the engine (same
logits bit for bit), and ConvNeXt-T at 224 in fp32 (the bars tests/test_gpu_fp32.py applies to ResNet50 and
ViT-B/16: rel-L2 <= 1e-4 against torch and identical top-1)."""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

SPECS = ["timm", "channels_first_ln", "reduce_mean_head"]
BATCHES = (1, 5)


def _rel_l2(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.fixture(scope="module")
def cn_models(native, tmp_path_factory):
    """spec -> (path, cfg, {B: (x, cpu executor logits, torch logits)}): the references are computed once"""
    import torch

    from die_amd.models import convnext as cn

    d = tmp_path_factory.mktemp("convnext_gpu")
    out = {}
    for spec in SPECS:
        cfg = cn.tiny_convnext_config(**cn.SPECS[spec])
        blob, w = cn.build_onnx(cfg)
        p = str(d / (spec + ".onnx"))
        open(p, "wb").write(blob)
        refs = {}
        for B in BATCHES:
            x = cn.synthetic_input(B, cfg, seed=20 + B)
            with torch.no_grad():
                t = cn.torch_forward(w, x, cfg, dtype=torch.float64).numpy()
            refs[B] = (x, native.cpu_run(p, x).reshape(B, -1), t)
        out[spec] = (p, cfg, refs)
    return out


@pytest.mark.parametrize("spec", SPECS)
@pytest.mark.parametrize("precision,tol", [("fp32", 1e-4), ("bf16", 3e-2)])
def test_tiny_convnext_matches_cpu_executor_and_torch(native, cn_models, spec, precision, tol):
    path, cfg, refs = cn_models[spec]
    eng = native.Engine(path, device="hip", max_batch=8, precision=precision, autotune=False)
    try:
        info = eng.refresh_info()
        assert info["name"].startswith("hip:gfx950"), info["name"]  # a plain HIP engine, no CPU island
        assert info["options"]["tiled_dwconv"] is True
        for B in BATCHES:
            x, cpu, tref = refs[B]
            got = eng.run(x.reshape(B, -1))
            assert got.shape == cpu.shape and np.isfinite(got).all()
            e_cpu, e_t = _rel_l2(got, cpu), _rel_l2(got.astype(np.float64), tref)
            print("convnext tiny %s %s B=%d rel-L2 vs cpu %.2e vs torch %.2e" % (spec, precision, B, e_cpu, e_t))
            assert e_cpu <= tol and e_t <= tol, (spec, precision, B, e_cpu, e_t)
            if precision == "fp32":
                assert (got.argmax(1) == cpu.argmax(1)).all() and (got.argmax(1) == tref.argmax(1)).all()
    finally:
        eng.close()


@pytest.mark.parametrize("spec", ["timm", "channels_first_ln"])
def test_tiled_kernel_off_gives_the_same_logits(native, cn_models, spec):
    """EngineOptions::tiled_dwconv = false sends the depthwise convs to gconv_kernel: the same bits"""
    path, cfg, refs = cn_models[spec]
    outs = {}
    for tiled in (True, False):
        eng = native.Engine(path, device="hip", max_batch=8, precision="fp32", autotune=False, tiled_dwconv=tiled)
        try:
            assert eng.refresh_info()["options"]["tiled_dwconv"] is tiled
            outs[tiled] = [eng.run(refs[B][0].reshape(B, -1)) for B in BATCHES]
        finally:
            eng.close()
    for a, b in zip(outs[True], outs[False]):
        assert np.array_equal(a.view(np.uint32), b.view(np.uint32))


def test_convnext_t_fp32_matches_torch(native, tmp_path):
    """ConvNeXt-T at 224, fp32, max batch 8: rel-L2 <= 1e-4 against torch fp32 and identical top-1 at B in {1, 7}"""
    import torch

    from die_amd.models import convnext as cn

    cfg = cn.ConvNeXtConfig()
    blob, w = cn.build_onnx(cfg)
    path = str(tmp_path / "convnext_t.onnx")
    open(path, "wb").write(blob)
    eng = native.Engine(path, device="hip", max_batch=8, precision="fp32")
    try:
        assert eng.refresh_info()["name"].startswith("hip:gfx950")
        for B in (1, 7):
            x = cn.synthetic_input(B, cfg, seed=50 + B)
            with torch.no_grad():
                ref = cn.torch_forward(w, x, cfg, device="cuda").double().cpu().numpy()
            got = eng.run(x.reshape(B, -1)).astype(np.float64)
            err = _rel_l2(got, ref)
            print("convnext_t B=%d rel-L2 fp32 %.2e" % (B, err))
            assert err <= 1e-4, (B, err)
            assert (got.argmax(1) == ref.argmax(1)).all(), B
    finally:
        eng.close()
