"""ConvNeXt-V2 through the HIP engine: the tiny config in both export forms of the GRN chain against the fp32
CPU executor and the torch oracle (the bars of tests/test_gpu_general.py and tests/test_gpu_convnext.py: fp32
rel-L2 <= 1e-4 and the same top-1, bf16 rel-L2 <= 3e-2), with one `grn` op per block in the engine's profile,
and ConvNeXt-V2-Atto at 224 in fp32 (ConvNeXt-T's bar: rel-L2 <= 1e-4 against torch fp32, identical top-1)."""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

SPECS = ["timm", "hf"]
BATCHES = (1, 5)


def _rel_l2(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.fixture(scope="module")
def v2_models(native, tmp_path_factory):
    """spec -> (path, cfg, {B: (x, cpu executor logits, torch logits)}): the references are computed once"""
    import torch

    from die_amd.models import convnextv2 as v2

    d = tmp_path_factory.mktemp("convnextv2_gpu")
    out = {}
    for spec in SPECS:
        cfg = v2.tiny_convnextv2_config(**v2.SPECS[spec])
        blob, w = v2.build_onnx(cfg)
        p = str(d / (spec + ".onnx"))
        open(p, "wb").write(blob)
        refs = {}
        for B in BATCHES:
            x = v2.synthetic_input(B, cfg, seed=20 + B)
            with torch.no_grad():
                t = v2.torch_forward(w, x, cfg, dtype=torch.float64).numpy()
            refs[B] = (x, native.cpu_run(p, x).reshape(B, -1), t)
        out[spec] = (p, cfg, refs)
    return out


@pytest.mark.parametrize("spec", SPECS)
@pytest.mark.parametrize("precision,tol", [("fp32", 1e-4), ("bf16", 3e-2)])
def test_tiny_convnextv2_matches_cpu_executor_and_torch(native, v2_models, spec, precision, tol):
    path, cfg, refs = v2_models[spec]
    eng = native.Engine(path, device="hip", max_batch=8, precision=precision, autotune=False)
    try:
        info = eng.refresh_info()
        assert info["name"].startswith("hip:gfx950"), info["name"]  # a plain HIP engine, no CPU island
        assert len(info.get("engine_stats", info)["grn"]) == sum(cfg.depths)
        for B in BATCHES:
            x, cpu, tref = refs[B]
            got = eng.run(x.reshape(B, -1))
            assert got.shape == cpu.shape and np.isfinite(got).all()
            e_cpu, e_t = _rel_l2(got, cpu), _rel_l2(got.astype(np.float64), tref)
            print("convnextv2 tiny %s %s B=%d rel-L2 vs cpu %.2e vs torch %.2e" % (spec, precision, B, e_cpu, e_t))
            assert e_cpu <= tol and e_t <= tol, (spec, precision, B, e_cpu, e_t)
            if precision == "fp32":
                assert (got.argmax(1) == cpu.argmax(1)).all() and (got.argmax(1) == tref.argmax(1)).all()
        prof = eng.profile(5, iters=2)
        grn = [o for o in prof["ops"] if o["kind"] == "grn"]
        assert len(grn) == sum(cfg.depths), [o["kind"] for o in prof["ops"]]
        assert sorted((o["C"], o["rows"]) for o in grn) == sorted(
            (4 * C, (cfg.image // 4 >> s) ** 2) for s, (d, C) in enumerate(zip(cfg.depths, cfg.dims)) for _ in range(d))
    finally:
        eng.close()


def test_convnextv2_atto_fp32_matches_torch(native, tmp_path):
    """ConvNeXt-V2-Atto at 224, fp32, max batch 8: rel-L2 <= 1e-4 against torch fp32 and identical top-1 at B in {1, 7}"""
    import torch

    from die_amd.models import convnextv2 as v2

    cfg = v2.atto_config()
    blob, w = v2.build_onnx(cfg)
    path = str(tmp_path / "convnextv2_atto.onnx")
    open(path, "wb").write(blob)
    eng = native.Engine(path, device="hip", max_batch=8, precision="fp32")
    try:
        assert eng.refresh_info()["name"].startswith("hip:gfx950")
        for B in (1, 7):
            x = v2.synthetic_input(B, cfg, seed=50 + B)
            with torch.no_grad():
                ref = v2.torch_forward(w, x, cfg, device="cuda").double().cpu().numpy()
            got = eng.run(x.reshape(B, -1)).astype(np.float64)
            err = _rel_l2(got, ref)
            print("convnextv2_atto B=%d rel-L2 fp32 %.2e" % (B, err))
            assert err <= 1e-4, (B, err)
            assert (got.argmax(1) == ref.argmax(1)).all(), B
    finally:
        eng.close()
