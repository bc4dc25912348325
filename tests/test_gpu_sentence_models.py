"""Sentence embedders (models/generic.py: sbert_ids, sbert_ids_hf, sbert_cls -- token ids in, a BERT
body, the masked mean over the visible tokens or the CLS token, L2 normalisation, one float vector
out) on the HIP engine against the fp32 CPU executor, at the bars of tests/test_gpu_token_models.py.
The engine must be the HIP engine itself, not the hybrid HIP + CPU one."""
import json
import urllib.request

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

NAMES = ["sbert_ids", "sbert_ids_hf", "sbert_cls"]
BATCHES = (1, 5, 8)


@pytest.fixture(scope="module")
def sentence_models(native, tmp_path_factory):
    from die_amd.models import generic as G

    d = tmp_path_factory.mktemp("sentence_gpu")
    out = {}
    for name in NAMES:
        p = str(d / (name + ".onnx"))
        open(p, "wb").write(G.build_onnx(name))
        out[name] = p
    return out


@pytest.fixture(scope="module")
def cpu_refs(native, sentence_models):
    """The CPU executor's outputs, once per (model, batch), shared by every test.  synthetic_lengths
    never gives an all-pad sample (tests/test_plan_sentence_pooling.py), so the oracle has no NaN."""
    from die_amd.models import generic as G

    refs = {}
    for name, path in sentence_models.items():
        for B in BATCHES:
            x = G.synthetic_input(name, B, seed=7)
            ref = native.cpu_run(path, x).reshape(B, -1)
            assert np.isfinite(ref).all()
            refs[name, B] = (x, ref)
    return refs


def _rel_l2(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("precision,tol", [("fp32", 1e-4), ("bf16", 3e-2)])
def test_sentence_model_matches_cpu_executor(native, sentence_models, cpu_refs, name, precision, tol):
    from die_amd.models import generic as G

    eng = native.Engine(sentence_models[name], device="hip", max_batch=8, precision=precision, autotune=False)
    try:
        info = eng.refresh_info()
        assert info["name"].startswith("hip:gfx950")  # not the hybrid engine
        assert info["input_kind"] == "token_ids" and info["vocab"] == 1000
        for B in BATCHES:
            x, ref = cpu_refs[name, B]
            got = eng.run(x.reshape(B, -1))
            assert got.shape == ref.shape == (B, G.SPECS[name]["dim"]) and np.isfinite(got).all()
            err = _rel_l2(got, ref)
            nerr = float(np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1.0).max())
            print(name, precision, B, "rel-L2 %.3e, | |v| - 1 | %.2e" % (err, nerr))
            assert err <= tol, (name, precision, B, err)
            if precision == "fp32":
                assert nerr <= 1e-5, (name, B, nerr)
    finally:
        eng.close()


@pytest.mark.parametrize("name", NAMES)
def test_a_sample_does_not_depend_on_its_neighbours(native, sentence_models, cpu_refs, name):
    eng = native.Engine(sentence_models[name], device="hip", max_batch=8, precision="fp32", autotune=False)
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


def test_sbert_ids_served_over_http_full_and_short_requests(native, sentence_models, cpu_refs):
    """A full-length request and a short id list (the device decode zero-fills the tail, 0 is the pad
    id) both answer D floats matching the CPU executor on the explicitly padded row."""
    from die_amd.models import generic as G

    path = sentence_models["sbert_ids"]
    S, D = G.SPECS["sbert_ids"]["seq"], G.SPECS["sbert_ids"]["dim"]
    x, ref = cpu_refs["sbert_ids", 5]
    wk = native.Worker(path, node_id="sbert", max_batch=8, engine={"device": "hip", "autotune": False})
    try:
        def infer(rid, values):
            body = json.dumps({"request_id": rid, "input_data": [float(v) for v in values]}).encode()
            out = json.loads(urllib.request.urlopen(urllib.request.Request(wk.url + "/infer", data=body), timeout=60).read())
            return np.array(out["output_data"], np.float32)

        full = infer("full", x[2])  # sample 2: full length, with a hole
        assert full.shape == (D,) and _rel_l2(full, ref[2]) <= 1e-4
        for i, L in ((1, 32), (3, 45), (4, 33)):
            assert (x[i, L:] == 0).all() and x[i, L - 1] != 0 and L < S
            short = infer("short%d" % i, x[i, :L])  # the first L ids only
            assert short.shape == (D,) and _rel_l2(short, ref[i]) <= 1e-4
        h = wk.health()["engine"]
        assert h["device"].startswith("hip") and h["input_kind"] == "token_ids"
    finally:
        wk.stop()
