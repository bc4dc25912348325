"""Grouped-query attention models (models/generic.py: gqa_enc, mqa_causal, gqa_hd128) on the HIP engine
against the fp32 CPU executor, at the bars of tests/test_gpu_rope_models.py: fp32 1e-4 rel-L2 and the
same top-1 for the classifiers, bf16 3e-2, unit length to 1e-5 in fp32 for the embedder.  The engine
must be the HIP engine itself, not the hybrid HIP + CPU one, and must answer what it answers on the
`expand_kv` multi-head twin."""
import json
import urllib.request

import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

NAMES = ["gqa_enc", "mqa_causal", "gqa_hd128"]
BATCHES = (1, 7, 32)


@pytest.fixture(scope="module")
def gqa_models(native, tmp_path_factory):
    from die_amd.models import generic as G

    d = tmp_path_factory.mktemp("gqa_gpu")
    out = {}
    for name in NAMES:
        for twin in (False, True):
            p = str(d / (name + ("_mha" if twin else "") + ".onnx"))
            open(p, "wb").write(G.BUILDERS[name](0, expand_kv=twin)[0])
            out[name, twin] = p
    return out


@pytest.fixture(scope="module")
def cpu_refs(native, gqa_models):
    """The CPU executor's outputs on one batch of 32 per model, shared by every test (samples are
    independent: the smaller batches are its first rows).  synthetic_lengths never gives an all-pad
    sample, so the oracle has no NaN."""
    from die_amd.models import generic as G

    refs = {}
    for name in NAMES:
        x = G.synthetic_input(name, max(BATCHES), seed=7)
        ref = native.cpu_run(gqa_models[name, False], x).reshape(len(x), -1)
        assert np.isfinite(ref).all()
        refs[name] = (x, ref)
    return refs


def _rel_l2(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("precision,tol", [("fp32", 1e-4), ("bf16", 3e-2)])
def test_model_matches_cpu_executor(native, gqa_models, cpu_refs, name, precision, tol):
    from die_amd.models import generic as G

    spec = G.SPECS[name]
    eng = native.Engine(gqa_models[name, False], device="hip", max_batch=32, precision=precision, autotune=False)
    try:
        info = eng.refresh_info()
        assert info["name"].startswith("hip:gfx950")  # not the hybrid engine
        x32, ref32 = cpu_refs[name]
        for B in BATCHES:
            x, ref = x32[:B], ref32[:B]
            got = eng.run(x.reshape(B, -1))
            assert got.shape == ref.shape and np.isfinite(got).all()
            err = _rel_l2(got, ref)
            print(name, precision, B, "rel-L2 %.3e" % err)
            assert err <= tol, (name, precision, B, err)
            if name == "gqa_enc":
                assert got.shape == (B, spec["dim"])
                nerr = float(np.abs(np.linalg.norm(got.astype(np.float64), axis=1) - 1.0).max())
                print(name, precision, B, "| |v| - 1 | %.2e" % nerr)
                if precision == "fp32":
                    assert nerr <= 1e-5, (name, B, nerr)
            elif precision == "fp32":
                assert got.shape == (B, spec["classes"]) and (got.argmax(1) == ref.argmax(1)).all()
        # the attention ops the plan promised run in the engine, with K / V heads as stored
        attn = [o for o in eng.profile(1, iters=1)["ops"] if o["kind"] == "attention"]
        assert len(attn) == spec["layers"] and all(o["kv_heads"] == spec["kv_heads"] for o in attn), attn
        assert all(o["causal"] == (name == "mqa_causal") and o["key_mask"] == (name == "gqa_enc") for o in attn), attn
    finally:
        eng.close()


@pytest.mark.parametrize("name", NAMES)
def test_engine_equals_its_expand_kv_twin(native, gqa_models, cpu_refs, name):
    """The twin stores every K / V head once per query head; the GQA plan reads them from the narrow buffer."""
    x32, _ = cpu_refs[name]
    x = x32[:7]
    outs = []
    for twin in (False, True):
        eng = native.Engine(gqa_models[name, twin], device="hip", max_batch=8, precision="fp32", autotune=False)
        try:
            assert eng.refresh_info()["name"].startswith("hip:gfx950")
            outs.append(eng.run(x.reshape(7, -1)))
        finally:
            eng.close()
    err = _rel_l2(outs[0], outs[1])
    print(name, "GQA engine vs expand_kv twin rel-L2 %.3e" % err)
    assert err <= 1e-4, (name, err)


def test_all_pad_sample_is_zero_and_leaves_its_neighbours_alone(native, gqa_models, cpu_refs):
    """A sample of pad ids only has no visible token: a zero vector (ONNX: NaN), and the samples around
    it answer what they answer without it."""
    eng = native.Engine(gqa_models["gqa_enc", False], device="hip", max_batch=8, precision="fp32", autotune=False)
    try:
        x32, ref32 = cpu_refs["gqa_enc"]
        with_pad = x32[:5].copy()
        with_pad[2] = 0
        got = eng.run(with_pad)
        assert np.isfinite(got).all() and (got[2] == 0).all()
        for i in (0, 1, 3, 4):
            err = _rel_l2(got[i], ref32[i])
            print("gqa_enc sample", i, "next to an all-pad sample rel-L2 %.3e" % err)
            assert err <= 1e-4, (i, err)
    finally:
        eng.close()


def test_gqa_enc_served_over_http_at_several_lengths(native, gqa_models, cpu_refs):
    """A full-length request and short id lists (the device decode zero-fills the tail, 0 is the pad id)
    answer D floats matching the CPU executor on the explicitly padded row."""
    from die_amd.models import generic as G

    S, D = G.SPECS["gqa_enc"]["seq"], G.SPECS["gqa_enc"]["dim"]
    x, ref = cpu_refs["gqa_enc"]
    wk = native.Worker(gqa_models["gqa_enc", False], node_id="gqa", max_batch=8, engine={"device": "hip", "autotune": False})
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
        assert [(o["heads"], o["kv_heads"], o["key_mask"], o["causal"]) for o in h["attention"]] == [(4, 2, True, False)] * 2
    finally:
        wk.stop()
