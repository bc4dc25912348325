"""Models with several graph inputs (input_ids, attention_mask, token_type_ids) on the CPU executor,
the oracle of tests/test_gpu_multi_input_models.py.  A request is the concatenation of the inputs'
per-sample elements in declaration order; the executor splits it by the declared dims and binds the
pieces by name.  Checked against the single-input twins (models/generic.py build_token_encoder with
inputs=("ids",): the same weights, the mask recomputed from the ids, one constant type row = row 0 of
the type table), whose path through the executor is the one it always had."""
import numpy as np
import pytest

NAMES = ["bert_hf3", "sbert_hf2"]
B = 5


@pytest.fixture(scope="module")
def paths(native, tmp_path_factory):
    from die_amd.models import generic as G

    d = tmp_path_factory.mktemp("multi_input_cpu")
    out = {}

    def save(key, blob):
        out[key] = str(d / (key.replace("/", "_") + ".onnx"))
        open(out[key], "wb").write(blob)

    for name in G.MULTI_INPUT:
        save(name, G.build_onnx(name))
        save(name + "/twin", G.build_token_encoder(spec=name, inputs=("ids",))[0])
    save("bert_ids_hf", G.build_onnx("bert_ids_hf"))
    save("sbert_ids_hf", G.build_onnx("sbert_ids_hf"))
    # bert_hf3_maskfirst's graph with the inputs declared ids, mask, types: bert_hf3's order
    save("maskfirst/ids_first", G.build_token_encoder(spec="bert_hf3_maskfirst", inputs=("ids", "mask", "types"))[0])
    for name in ("mlp", "bert_ids"):
        save(name, G.build_onnx(name))
    return out


def _rel_l2(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


def _request(G, name, seg):
    return np.concatenate([seg[r] for r in G.SPECS[name]["inputs"]], axis=1).astype(np.float32)


@pytest.mark.parametrize("name", NAMES)
def test_equals_the_single_input_twin_when_the_mask_is_ids_gt_0_and_types_are_0(native, paths, name):
    """The same arithmetic on the same values: bit-equal in practice, rel-L2 <= 1e-6 is the bar.  The
    twins: the builder's single-input variant of the same spec, and the in-tree bert_ids_hf /
    sbert_ids_hf, which draw the same weights."""
    from die_amd.models import generic as G

    ids = G.synthetic_ids(name, B, np.random.default_rng(11))  # pads are id 0, a hole in sample 2
    assert (ids == 0).any() and (ids[:, 0] != 0).all()
    seg = dict(ids=ids, mask=(ids > 0).astype(np.float32), types=np.zeros_like(ids))
    got = native.cpu_run(paths[name], _request(G, name, seg))
    for twin in (name + "/twin", {"bert_hf3": "bert_ids_hf", "sbert_hf2": "sbert_ids_hf"}[name]):
        ref = native.cpu_run(paths[twin], ids)
        assert got.shape == ref.shape and np.isfinite(got).all()
        err = _rel_l2(got, ref)
        print(name, twin, "rel-L2 %.3e" % err)
        assert err <= 1e-6, (name, twin, err)


@pytest.mark.parametrize("name", NAMES)
def test_the_mask_is_read_from_the_mask_input(native, paths, name):
    """Random non-zero ids in the hidden positions of the multi-input model, zeros there for the twin
    (whose visible ids are all non-zero): the CLS logits and the masked mean depend on the visible
    keys only, so the two agree -- unless the mask were still derived from the ids."""
    from die_amd.models import generic as G

    s = G.SPECS[name]
    rng = np.random.default_rng(5)
    ids = rng.integers(1, s["vocab"], size=(B, s["seq"])).astype(np.float32)
    mask = np.zeros_like(ids)
    for i, n in enumerate(G.synthetic_lengths(name, B)):
        mask[i, :n] = 1
        if i % 3 == 2 and n >= 3:
            mask[i, n // 2] = 0
    assert ((mask == 0) & (ids != 0)).any()
    seg = dict(ids=ids, mask=mask, types=np.zeros_like(ids))
    got = native.cpu_run(paths[name], _request(G, name, seg))
    ref = native.cpu_run(paths[name + "/twin"], ids * mask)
    err = _rel_l2(got, ref)
    print(name, "hidden ids random vs zero: rel-L2 %.3e" % err)
    assert err <= 1e-6, (name, err)
    # and the hidden ids are really ignored, the mask really used: all-visible gives another answer
    seg["mask"] = np.ones_like(ids)
    assert _rel_l2(native.cpu_run(paths[name], _request(G, name, seg)), ref) > 1e-3


def test_types_select_the_row_of_the_type_table(native, paths):
    from die_amd.models import generic as G

    x = G.synthetic_input("bert_hf3", B)
    S = G.SPECS["bert_hf3"]["seq"]
    assert (x[:, 2 * S:] == 1).any()
    y = native.cpu_run(paths["bert_hf3"], x)
    x0 = x.copy()
    x0[:, 2 * S:] = 0
    assert _rel_l2(native.cpu_run(paths["bert_hf3"], x0), y) > 1e-3


def test_declaration_order_only_moves_the_segments(native, paths):
    """bert_hf3_maskfirst (declared mask, types, ids) fed mask | types | ids equals the same graph
    declared in bert_hf3's order fed ids | mask | types."""
    from die_amd.models import generic as G

    name = "bert_hf3_maskfirst"
    S = G.SPECS[name]["seq"]
    x = G.synthetic_input(name, B)  # mask | types | ids
    assert x.shape == (B, 3 * S) and set(np.unique(x[:, :2 * S])) <= {0.0, 1.0} and x[:, 2 * S:].max() > 1
    mask, types, ids = x[:, :S], x[:, S:2 * S], x[:, 2 * S:]
    a = native.cpu_run(paths[name], x)
    b = native.cpu_run(paths["maskfirst/ids_first"], np.concatenate([ids, mask, types], axis=1))
    assert a.shape == (B, G.SPECS[name]["classes"])
    assert _rel_l2(a, b) <= 1e-6 and np.array_equal(a, b)
    assert native.model_inputs(paths[name])["request_shape"] == [1, 3, S]


def test_synthetic_requests_prove_the_mask_input(native):
    """What models/generic.py synthetic_request promises: hidden positions hold non-zero ids, every
    third sample has a hole, a visible token has id 0, types switch at half the length."""
    from die_amd.models import generic as G

    for name in G.MULTI_INPUT:
        s = G.SPECS[name]
        S, order = s["seq"], s["inputs"]
        x = G.synthetic_input(name, 8)
        assert x.shape == (8,) + G.input_shape(name) == (8, len(order) * S) and x.dtype == np.float32
        seg = {r: x[:, k * S:(k + 1) * S] for k, r in enumerate(order)}
        for i, n in enumerate(G.synthetic_lengths(name, 8)):
            m, ids = seg["mask"][i], seg["ids"][i]
            assert (m[n:] == 0).all() and m[n - 1] == 1 and (ids[m == 0] != 0).all()
            assert (m[:n] == 0).sum() == (1 if i % 3 == 2 and n >= 3 else 0)
            if n >= 3:
                assert ((ids == 0) & (m == 1)).sum() == 1
            if "types" in seg:
                assert (seg["types"][i, :n // 2] == 0).all() and (seg["types"][i, n // 2:n] == 1).all()


@pytest.mark.parametrize("name,last", [("mlp", "prob"), ("bert_ids", "classifier")])
def test_single_input_models_run_as_before(native, paths, name, last):
    """One graph input: the whole tensor is bound as it is.  cpu_run's output is the value of the last
    node, and the request description is that input alone."""
    from die_amd.models import generic as G

    x = G.synthetic_input(name, 3)
    y = native.cpu_run(paths[name], x)
    assert np.array_equal(y, native.cpu_run_value(paths[name], x, last))
    mi = native.model_inputs(paths[name])
    assert len(mi["inputs"]) == 1 and mi["inputs"][0]["offset"] == 0
    assert mi["input_numel"] == int(np.prod(G.input_shape(name))) and mi["request_shape"] == [1] + list(G.input_shape(name))
    assert mi["inputs"][0]["role"] == ("ids" if name == "bert_ids" else "activations")


def test_a_wrongly_sized_request_is_an_error(native, paths):
    from die_amd.models import generic as G

    S = G.SPECS["bert_hf3"]["seq"]
    with pytest.raises(native.NativeError, match="3 inputs"):
        native.cpu_run(paths["bert_hf3"], np.zeros((2, S), np.float32))


@pytest.mark.parametrize("name", ["bert_hf3", "sbert_hf2", "bert_hf3_maskfirst"])
def test_cpu_engine_shape_and_dp_arena_use_every_input(native, paths, name):
    """The CPU engine reports [1, K, S] and takes K * S numbers per request; a DP arena item holds as
    many floats.  A short request is zero-filled: its missing mask hides everything."""
    from die_amd.models import generic as G

    s = G.SPECS[name]
    K, S = len(s["inputs"]), s["seq"]
    mi = native.model_inputs(paths[name])
    assert mi["input_numel"] == K * S
    assert [(e["role"], e["offset"], e["numel"]) for e in mi["inputs"]] == [
        ({"ids": "ids", "mask": "mask", "types": "types"}[r] if name != "bert_hf3_maskfirst" else
         {"mask": "mask", "types": "ids", "ids": "types"}[r], k * S, S) for k, r in enumerate(s["inputs"])]
    plan = native.dp_arena_plan(mi["input_numel"], 2, max_batch=8, device="cpu")
    assert plan["item_bytes"] == K * S * 4
    eng = native.Engine(paths[name], device="cpu", max_batch=4)
    try:
        info = eng.refresh_info()
        assert info["name"] == "cpu" and info["input_shape"] == [1, K, S] and eng.input_numel == K * S
        assert [e["role"] for e in info["inputs"]] == [e["role"] for e in mi["inputs"]]
        x = G.synthetic_input(name, 3)
        assert _rel_l2(eng.run(x), native.cpu_run(paths[name], x).reshape(3, -1)) <= 1e-6
    finally:
        eng.close()
