"""Models whose attention carries a constant bias or mask (models/generic.py: gpt_causal,
bert_relpos, bert_window, bert_keymask) on the HIP engine against the fp32 CPU executor, at the
bars of tests/test_gpu_general.py.  The engine must be the HIP engine itself: the hybrid HIP + CPU
engine would pass the numerics with the attention on the CPU."""
import json
import urllib.request

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

MASKED = ["gpt_causal", "bert_relpos", "bert_window", "bert_keymask"]


@pytest.fixture(scope="module")
def masked_models(native, tmp_path_factory):
    from die_amd.models import generic as G

    d = tmp_path_factory.mktemp("masked_gpu")
    out = {}
    for name in MASKED:
        p = str(d / (name + ".onnx"))
        open(p, "wb").write(G.build_onnx(name))
        out[name] = p
    return out


@pytest.fixture(scope="module")
def cpu_refs(native, masked_models):
    """The CPU executor's outputs, computed once per (model, batch) and shared by both precisions."""
    from die_amd.models import generic as G

    refs = {}
    for name, path in masked_models.items():
        for B in (1, 5, 8):
            x = G.synthetic_input(name, B, seed=B)
            refs[name, B] = (x, native.cpu_run(path, x).reshape(B, -1))
    return refs


def _rel_l2(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("name", MASKED)
@pytest.mark.parametrize("precision,tol", [("fp32", 1e-4), ("bf16", 3e-2)])
def test_masked_model_matches_cpu_executor(native, masked_models, cpu_refs, name, precision, tol):
    eng = native.Engine(masked_models[name], device="hip", max_batch=8, precision=precision, autotune=False)
    try:
        assert eng.refresh_info()["name"].startswith("hip:gfx950")
        for B in (1, 5, 8):
            x, ref = cpu_refs[name, B]
            got = eng.run(x.reshape(B, -1))
            assert got.shape == ref.shape and np.isfinite(got).all()
            err = _rel_l2(got, ref)
            print(name, precision, B, "rel-L2 %.3e" % err)
            assert err <= tol, (name, precision, B, err)
            if precision == "fp32":
                assert (got.argmax(1) == ref.argmax(1)).all()
    finally:
        eng.close()


def test_gpt_causal_served_over_http(native, masked_models, cpu_refs):
    path = masked_models["gpt_causal"]
    wk = native.Worker(path, node_id="gpt", max_batch=8, engine={"device": "hip", "autotune": False})
    try:
        x, ref = cpu_refs["gpt_causal", 5]
        for i in range(3):
            body = json.dumps({"request_id": "g%d" % i, "input_data": [float(v) for v in x[i]]}).encode()
            out = json.loads(urllib.request.urlopen(urllib.request.Request(wk.url + "/infer", data=body),
                                                    timeout=60).read())
            assert _rel_l2(np.array(out["output_data"], np.float32), ref[i]) <= 1e-4
        assert wk.health()["engine"]["device"].startswith("hip")
    finally:
        wk.stop()
