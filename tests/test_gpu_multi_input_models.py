"""Token models with attention_mask / token_type_ids graph inputs (models/generic.py: bert_hf3,
sbert_hf2, bert_hf3_maskfirst) on the HIP engine against the fp32 CPU executor, at the bars of
tests/test_gpu_token_models.py.  A request row is the inputs' [S] one after the other in declaration
order.  The synthetic requests hold non-zero ids in hidden positions and a visible id 0, so a mask
still derived from the ids fails here.  The engine must be the HIP engine itself, not the hybrid or
the CPU engine."""
import json
import urllib.request

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

NAMES = ["bert_hf3", "sbert_hf2", "bert_hf3_maskfirst"]
BATCHES = (1, 5, 8)


@pytest.fixture(scope="module")
def multi_models(native, tmp_path_factory):
    from die_amd.models import generic as G

    d = tmp_path_factory.mktemp("multi_input_gpu")
    out = {}
    for name in NAMES:
        out[name] = str(d / (name + ".onnx"))
        open(out[name], "wb").write(G.build_onnx(name))
    return out


@pytest.fixture(scope="module")
def cpu_refs(native, multi_models):
    """The CPU executor's outputs, once per (model, batch), shared by every test."""
    from die_amd.models import generic as G

    refs = {}
    for name, path in multi_models.items():
        for B in BATCHES:
            x = G.synthetic_input(name, B, seed=7)
            refs[name, B] = (x, native.cpu_run(path, x).reshape(B, -1))
    return refs


def _rel_l2(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("precision,tol", [("fp32", 1e-4), ("bf16", 3e-2)])
def test_multi_input_model_matches_cpu_executor(native, multi_models, cpu_refs, name, precision, tol):
    from die_amd.models import generic as G

    spec = G.SPECS[name]
    K, S = len(spec["inputs"]), spec["seq"]
    eng = native.Engine(multi_models[name], device="hip", max_batch=8, precision=precision, autotune=False)
    try:
        info = eng.refresh_info()
        assert info["name"].startswith("hip:gfx950")  # not the hybrid engine, not the CPU engine
        assert info["input_kind"] == "token_ids" and "mask input" in info["pad_compare"]
        assert info["input_shape"] == [1, K, S] and eng.input_numel == K * S
        assert sorted(e["role"] for e in info["inputs"]) == sorted({"ids": "ids", "mask": "mask", "types": "types"}[r]
                                                                    for r in spec["inputs"])
        assert [e["offset"] for e in info["inputs"]] == [k * S for k in range(K)]
        for B in BATCHES:
            x, ref = cpu_refs[name, B]
            got = eng.run(x)
            assert got.shape == ref.shape and np.isfinite(got).all()
            err = _rel_l2(got, ref)
            print(name, precision, B, "rel-L2 %.3e" % err)
            assert err <= tol, (name, precision, B, err)
            if precision == "fp32" and "classes" in spec:
                assert (got.argmax(1) == ref.argmax(1)).all()
            if precision == "fp32" and "classes" not in spec:
                assert np.abs(np.linalg.norm(got, axis=1) - 1).max() <= 1e-5
    finally:
        eng.close()


@pytest.mark.parametrize("name", NAMES)
def test_a_sample_does_not_depend_on_its_neighbours(native, multi_models, cpu_refs, name):
    """Sample i of the batch of 5 equals the sample run alone: the segments are read with the row
    pitch K * S, and a neighbour's mask (its key data, its shorter tile walk) must not leak."""
    eng = native.Engine(multi_models[name], device="hip", max_batch=8, precision="fp32", autotune=False)
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


def _infer(wk, rid, values):
    body = json.dumps({"request_id": rid, "input_data": [float(v) for v in values]}).encode()
    out = json.loads(urllib.request.urlopen(urllib.request.Request(wk.url + "/infer", data=body), timeout=60).read())
    return np.array(out["output_data"], np.float32)


def test_served_over_http_full_and_ids_only_requests(native, multi_models, cpu_refs):
    """A full request carries K * S numbers, ids | mask | types.  A request carrying only the first S
    numbers (the ids) is zero-filled like any short request: its mask is all 0, every key hidden.
    For the embedder that is the documented all-padding answer, a vector of zeros (the masked mean of
    no token is 0 / max(0, 1e-9), and 0 / max(||0||, eps) = 0), on the HIP worker and on a CPU worker
    alike.  (A classifier has no such common answer -- with every key hidden the CPU executor's
    softmax is uniform where the device writes zero rows, DESIGN §9 -- so the embedder is the one
    checked.)"""
    from die_amd.models import generic as G

    S = G.SPECS["bert_hf3"]["seq"]
    x, ref = cpu_refs["bert_hf3", 5]
    wk = native.Worker(multi_models["bert_hf3"], node_id="hf3", max_batch=8, engine={"device": "hip", "autotune": False})
    try:
        for i in (1, 2):  # length 32; full length with a hole
            assert _rel_l2(_infer(wk, "full%d" % i, x[i]), ref[i]) <= 1e-4
        h = wk.health()["engine"]
        assert h["device"].startswith("hip") and h["input_kind"] == "token_ids" and h["vocab"] == 1000
        assert [(e["name"], e["role"], e["offset"], e["numel"]) for e in h["inputs"]] == [
            ("input_ids", "ids", 0, S), ("attention_mask", "mask", S, S), ("token_type_ids", "types", 2 * S, S)]
    finally:
        wk.stop()
    S = G.SPECS["sbert_hf2"]["seq"]
    x, ref = cpu_refs["sbert_hf2", 5]
    for device in ("hip", "cpu"):
        wk = native.Worker(multi_models["sbert_hf2"], node_id="hf2" + device, max_batch=8,
                           engine={"device": device, "autotune": False})
        try:
            assert _rel_l2(_infer(wk, "full", x[3]), ref[3]) <= 1e-4
            short = _infer(wk, "ids_only", x[3, :S])
            assert short.shape == ref[3].shape and (short == 0).all(), (device, short[:4])
            assert [e["role"] for e in wk.health()["engine"]["inputs"]] == ["ids", "mask"]
        finally:
            wk.stop()


def test_run_text_feeds_the_segments(native, multi_models, cpu_refs):
    """The device JSON decode writes the flat request: all K * S numbers of each sample as text."""
    name = "bert_hf3_maskfirst"
    x, ref = cpu_refs[name, 5]
    eng = native.Engine(multi_models[name], device="hip", max_batch=8, precision="fp32", autotune=False)
    try:
        texts = [",".join("%d" % v for v in row).encode() for row in x]
        got, status = eng.run_text(texts)
        assert status.tolist() == [0] * 5
        assert _rel_l2(got, ref) <= 1e-4 and np.array_equal(got, eng.run(x))
    finally:
        eng.close()
