"""Rotary / RMSNorm models (models/generic.py: rope_bert, rope_bert_nshd, llama_enc, llama_enc_rmsnode)
on the HIP engine against the fp32 CPU executor.  Classifiers at the bars of
tests/test_gpu_masked_models.py (fp32 1e-4 rel-L2 and the same top-1, bf16 3e-2), embedders at those of
tests/test_gpu_sentence_models.py (the same two, and unit length to 1e-5 in fp32).  The engine must
be the HIP engine itself, not the hybrid HIP + CPU one."""
import json
import urllib.request

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

CLASSIFIERS = ["rope_bert", "rope_bert_nshd"]
EMBEDDERS = ["llama_enc", "llama_enc_rmsnode"]
BATCHES = (1, 5)


@pytest.fixture(scope="module")
def rope_models(native, tmp_path_factory):
    from die_amd.models import generic as G

    d = tmp_path_factory.mktemp("rope_gpu")
    out = {}
    for name in CLASSIFIERS + EMBEDDERS:
        p = str(d / (name + ".onnx"))
        open(p, "wb").write(G.build_onnx(name))
        out[name] = p
    return out


@pytest.fixture(scope="module")
def cpu_refs(native, rope_models):
    """The CPU executor's outputs, once per (model, batch), shared by every test.  synthetic_lengths
    never gives an all-pad sample, so the oracle has no NaN."""
    from die_amd.models import generic as G

    refs = {}
    for name, path in rope_models.items():
        for B in BATCHES:
            x = G.synthetic_input(name, B, seed=7)
            ref = native.cpu_run(path, x).reshape(B, -1)
            assert np.isfinite(ref).all()
            refs[name, B] = (x, ref)
    return refs


def _rel_l2(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _kinds(eng):
    return [o["kind"] for o in eng.profile(1, iters=1)["ops"]]


@pytest.mark.parametrize("name", CLASSIFIERS + EMBEDDERS)
@pytest.mark.parametrize("precision,tol", [("fp32", 1e-4), ("bf16", 3e-2)])
def test_model_matches_cpu_executor(native, rope_models, cpu_refs, name, precision, tol):
    from die_amd.models import generic as G

    spec = G.SPECS[name]
    eng = native.Engine(rope_models[name], device="hip", max_batch=8, precision=precision, autotune=False)
    try:
        info = eng.refresh_info()
        assert info["name"].startswith("hip:gfx950")  # not the hybrid engine
        if name in EMBEDDERS:
            assert info["input_kind"] == "token_ids" and info["vocab"] == spec["vocab"]
        for B in BATCHES:
            x, ref = cpu_refs[name, B]
            got = eng.run(x.reshape(B, -1))
            assert got.shape == ref.shape and np.isfinite(got).all()
            err = _rel_l2(got, ref)
            print(name, precision, B, "rel-L2 %.3e" % err)
            assert err <= tol, (name, precision, B, err)
            if name in EMBEDDERS:
                assert got.shape == (B, spec["dim"])
                nerr = float(np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1.0).max())
                print(name, precision, B, "| |v| - 1 | %.2e" % nerr)
                if precision == "fp32":
                    assert nerr <= 1e-5, (name, B, nerr)
            elif precision == "fp32":
                assert got.shape == (B, spec["classes"]) and (got.argmax(1) == ref.argmax(1)).all()
        # the ops the plan promised run in the engine: two rope launches per layer
        kinds = _kinds(eng)
        assert kinds.count("rope") == 2 * spec["layers"], kinds
    finally:
        eng.close()


@pytest.mark.parametrize("name", EMBEDDERS)
def test_all_pad_sample_is_zero_and_leaves_its_neighbours_alone(native, rope_models, cpu_refs, name):
    """A sample of pad ids only has no visible token: the documented answer is a zero vector (ONNX: NaN),
    and the samples around it answer what they answer without it."""
    eng = native.Engine(rope_models[name], device="hip", max_batch=8, precision="fp32", autotune=False)
    try:
        x, ref = cpu_refs[name, 5]
        with_pad = x.copy()
        with_pad[2] = 0
        got = eng.run(with_pad)
        assert np.isfinite(got).all() and (got[2] == 0).all()
        for i in (0, 1, 3, 4):
            err = _rel_l2(got[i], ref[i])
            print(name, "sample", i, "next to an all-pad sample rel-L2 %.3e" % err)
            assert err <= 1e-4, (name, i, err)
    finally:
        eng.close()


def test_llama_enc_served_over_http_at_several_lengths(native, rope_models, cpu_refs):
    """A full-length request and short id lists (the device decode zero-fills the tail, 0 is the pad id)
    answer D floats matching the CPU executor on the explicitly padded row."""
    from die_amd.models import generic as G

    path = rope_models["llama_enc"]
    S, D = G.SPECS["llama_enc"]["seq"], G.SPECS["llama_enc"]["dim"]
    x, ref = cpu_refs["llama_enc", 5]
    wk = native.Worker(path, node_id="llama", max_batch=8, engine={"device": "hip", "autotune": False})
    try:
        def infer(rid, values):
            body = json.dumps({"request_id": rid, "input_data": [float(v) for v in values]}).encode()
            out = json.loads(urllib.request.urlopen(urllib.request.Request(wk.url + "/infer", data=body), timeout=60).read())
            return np.array(out["output_data"], np.float32)

        full = infer("full", x[2])  # sample 2: full length, with a hole
        assert full.shape == (D,) and _rel_l2(full, ref[2]) <= 1e-4
        for i, L in ((0, 1), (1, 32), (3, 45), (4, 33)):
            assert (x[i, L:] == 0).all() and x[i, L - 1] != 0 and L < S
            short = infer("short%d" % i, x[i, :L])  # the first L ids only
            assert short.shape == (D,) and _rel_l2(short, ref[i]) <= 1e-4
        h = wk.health()["engine"]
        assert h["device"].startswith("hip") and h["input_kind"] == "token_ids"
    finally:
        wk.stop()
