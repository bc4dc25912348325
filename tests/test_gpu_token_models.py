"""Token-id models (models/generic.py: bert_ids, bert_ids_hf -- embedding lookup on the graph input,
attention masked by the request's own padding) on the HIP engine against the fp32 CPU executor, at
the bars of tests/test_gpu_general.py.  The engine must be the HIP engine itself: the hybrid HIP + CPU
engine would pass the numerics with the lookup and the attention on the CPU."""
import json
import urllib.request

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

NAMES = ["bert_ids", "bert_ids_hf"]
BATCHES = (1, 5, 8)


@pytest.fixture(scope="module")
def token_models(native, tmp_path_factory):
    from die_amd.models import generic as G

    d = tmp_path_factory.mktemp("token_gpu")
    out = {}
    for name in NAMES:
        p = str(d / (name + ".onnx"))
        open(p, "wb").write(G.build_onnx(name))
        out[name] = p
    return out


@pytest.fixture(scope="module")
def cpu_refs(native, token_models):
    """The CPU executor's outputs, computed once per (model, batch) and shared by every test: batch B
    is the synthetic batch (lengths 1, 32, S, 45, 33 in turn, a hole in every third sample); the
    key (name, 5, i) is sample i of the batch of 5 run alone."""
    from die_amd.models import generic as G

    refs = {}
    for name, path in token_models.items():
        for B in BATCHES:
            x = G.synthetic_input(name, B, seed=7)
            refs[name, B] = (x, native.cpu_run(path, x).reshape(B, -1))
    return refs


def _rel_l2(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("precision,tol", [("fp32", 1e-4), ("bf16", 3e-2)])
def test_token_model_matches_cpu_executor(native, token_models, cpu_refs, name, precision, tol):
    eng = native.Engine(token_models[name], device="hip", max_batch=8, precision=precision, autotune=False)
    try:
        info = eng.refresh_info()
        assert info["name"].startswith("hip:gfx950")  # not the hybrid engine
        assert info["input_kind"] == "token_ids" and info["vocab"] == 1000 and "0" in info["pad_compare"]
        for B in BATCHES:
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


@pytest.mark.parametrize("name", NAMES)
def test_a_sample_does_not_depend_on_its_neighbours(native, token_models, cpu_refs, name):
    """At B = 5 a sample's logits are those of the same sample run alone: a neighbour's padding (its
    key data, its shorter tile walk) must not leak."""
    eng = native.Engine(token_models[name], device="hip", max_batch=8, precision="fp32", autotune=False)
    try:
        x, _ = cpu_refs[name, 5]
        batch = eng.run(x)
        for i in range(5):
            alone = eng.run(x[i:i + 1])
            err = _rel_l2(batch[i], alone[0])
            print(name, "sample", i, "batch vs alone rel-L2 %.3e" % err)
            assert err <= 1e-4, (name, i, err)
    finally:
        eng.close()


def test_bert_ids_served_over_http_full_and_short_requests(native, token_models, cpu_refs):
    """One request carries all S ids; a second only the first L (the device decode zero-fills the tail
    of a short input, and 0 is the pad id): both answer as the CPU executor does on the explicitly
    padded row."""
    from die_amd.models import generic as G

    path = token_models["bert_ids"]
    S = G.SPECS["bert_ids"]["seq"]
    x, ref = cpu_refs["bert_ids", 5]
    wk = native.Worker(path, node_id="ids", max_batch=8, engine={"device": "hip", "autotune": False})
    try:
        def infer(rid, values):
            body = json.dumps({"request_id": rid, "input_data": [float(v) for v in values]}).encode()
            out = json.loads(urllib.request.urlopen(urllib.request.Request(wk.url + "/infer", data=body), timeout=60).read())
            return np.array(out["output_data"], np.float32)

        # sample 2: full length (with a hole); samples 1, 3, 4: lengths 32, 45, 33
        assert _rel_l2(infer("full", x[2]), ref[2]) <= 1e-4
        for i, L in ((1, 32), (3, 45), (4, 33)):
            assert (x[i, L:] == 0).all() and x[i, L - 1] != 0 and L < S
            assert _rel_l2(infer("padded%d" % i, x[i]), ref[i]) <= 1e-4  # all S ids, the tail explicit zeros
            assert _rel_l2(infer("short%d" % i, x[i, :L]), ref[i]) <= 1e-4  # the first L ids only
        h = wk.health()["engine"]
        assert h["device"].startswith("hip") and h["input_kind"] == "token_ids" and h["vocab"] == 1000
    finally:
        wk.stop()
