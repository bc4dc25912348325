"""GroupNorm / InstanceNorm models (models/groupnorm.py: gn_resnet, gn_resnet_node, gn_decoder, inorm_net) on
the HIP engine against the fp32 CPU executor, at the bars of tests/test_gpu_fuzz.py (arbitrary generated
graphs): fp32 rel-L2 <= 2e-4, and the same top-1 for the classifier; bf16 at 1e-2.  The engine must be the
HIP engine itself, not the hybrid HIP + CPU one; a sample's answer must not depend on its batch, and the
captured graph must give the bits of the eager launches."""
import numpy as np
import pytest

from conftest import gpu_available

pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not gpu_available(), reason="needs a GPU")]

NAMES = ["gn_resnet", "gn_resnet_node", "gn_decoder", "inorm_net"]
BATCHES = (1, 3, 8)


@pytest.fixture(scope="module")
def gn_models(native, tmp_path_factory):
    from die_amd.models import groupnorm as M

    d = tmp_path_factory.mktemp("groupnorm_gpu")
    out = {}
    for name in NAMES:
        p = str(d / (name + ".onnx"))
        open(p, "wb").write(M.BUILDERS[name](0)[0])
        out[name] = p
    return out


@pytest.fixture(scope="module")
def cpu_refs(native, gn_models):
    """The CPU executor's outputs, once per (model, batch), shared by every test"""
    from die_amd.models import groupnorm as M

    refs = {}
    for name, path in gn_models.items():
        for B in BATCHES:
            x = M.synthetic_input(name, B, seed=7)
            ref = native.cpu_run(path, x).reshape(B, -1)
            assert np.isfinite(ref).all()
            refs[name, B] = (x.reshape(B, -1), ref)
    return refs


def _rel_l2(a, b):
    return float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-30))


@pytest.mark.parametrize("name", NAMES)
@pytest.mark.parametrize("precision,tol", [("fp32", 2e-4), ("bf16", 1e-2)])
def test_model_matches_cpu_executor(native, gn_models, cpu_refs, name, precision, tol):
    from die_amd.models import groupnorm as M

    eng = native.Engine(gn_models[name], device="hip", max_batch=8, precision=precision, autotune=False)
    try:
        info = eng.refresh_info()
        assert info["name"].startswith("hip:gfx950"), info["name"]  # not the hybrid engine
        for B in BATCHES:
            x, ref = cpu_refs[name, B]
            got = eng.run(x)
            assert got.shape == ref.shape and np.isfinite(got).all()
            err = _rel_l2(got, ref)
            print(name, precision, B, "rel-L2 %.3e" % err)
            assert err <= tol, (name, precision, B, err)
            if precision == "fp32" and name.startswith("gn_resnet"):
                assert (got.argmax(1) == ref.argmax(1)).all(), (name, B)
        # the ops the plan promised run in the engine, with their geometry in the profile and the stats
        ops = [o for o in eng.profile(1, iters=1)["ops"] if o["kind"] == "groupnorm"]
        assert [(o["groups"], o["channels"], o["act"]) for o in ops] == M.EXPECTED_NORMS[name]
        st = info.get("engine_stats", info)
        assert [(o["groups"], o["channels"], o["act"]) for o in st["groupnorm"]] == M.EXPECTED_NORMS[name]
    finally:
        eng.close()


@pytest.mark.parametrize("name", NAMES)
def test_sample_bits_do_not_depend_on_the_batch(native, gn_models, cpu_refs, name):
    """a batch-3 run gives each sample the bits it gets alone"""
    eng = native.Engine(gn_models[name], device="hip", max_batch=8, precision="fp32", autotune=False)
    try:
        x, _ = cpu_refs[name, 3]
        got = eng.run(x)
        for i in range(3):
            np.testing.assert_array_equal(eng.run(x[i:i + 1])[0], got[i], err_msg="%s sample %d" % (name, i))
    finally:
        eng.close()


@pytest.mark.parametrize("name", NAMES)
def test_graph_replay_equals_eager(native, gn_models, cpu_refs, name):
    base = dict(device="hip", max_batch=8, precision="fp32", autotune=False, tune_cache="")
    a = native.Engine(gn_models[name], use_graphs=True, **base)
    b = native.Engine(gn_models[name], use_graphs=False, **base)
    try:
        assert a.refresh_info()["hip_graphs"] is True and b.refresh_info()["hip_graphs"] is False
        for B in BATCHES:
            x, _ = cpu_refs[name, B]
            ya = a.run(x)
            np.testing.assert_array_equal(ya, a.run(x))
            np.testing.assert_array_equal(ya, b.run(x))
    finally:
        a.close()
        b.close()
