"""CPU executor (the oracle of the GPU tests): ReduceL2 and LpNormalization against numpy float64, and
the sentence-transformers pooling tail (masked mean over the visible tokens, then F.normalize) as a
small graph of its own.  No GPU."""
import numpy as np
import pytest


def _run(native, tmp_path, g, x, name):
    p = str(tmp_path / (name + ".onnx"))
    open(p, "wb").write(g.model_proto(opset=17))
    return native.cpu_run(p, x)


def _reduce_l2_ref(x, axes, keep):
    return np.sqrt((x.astype(np.float64) ** 2).sum(axis=tuple(axes), keepdims=bool(keep)))


@pytest.mark.parametrize("shape,axes", [((5, 12), [1]), ((5, 12), [-1]), ((5, 12), [0]), ((3, 7, 10), [2]),
                                        ((3, 7, 10), [-1]), ((3, 7, 10), [-2]), ((3, 7, 10), [1, 2]),
                                        ((3, 7, 10), [-3])])
@pytest.mark.parametrize("keep", [0, 1])
@pytest.mark.parametrize("axes_as_input", [False, True])
def test_reduce_l2(native, tmp_path, shape, axes, keep, axes_as_input):
    from die_amd.utils.onnx_writer import GraphBuilder

    x = np.random.default_rng(len(shape) * 10 + keep).standard_normal(shape).astype(np.float32)
    g = GraphBuilder(name="rl2")
    v = g.input("x", ["N"] + list(shape[1:]))
    if axes_as_input:
        y = g.node("ReduceL2", [v, g.const(np.array(axes, np.int64), "axes")], name="norm", keepdims=keep)
    else:
        y = g.node("ReduceL2", [v], name="norm", axes=axes, keepdims=keep)
    ref = _reduce_l2_ref(x, axes, keep)
    g.output(y, ["N"] + list(ref.shape[1:]))
    got = _run(native, tmp_path, g, x, "rl2")
    assert got.shape == ref.shape, (got.shape, ref.shape)
    np.testing.assert_allclose(got, ref, rtol=2e-6, atol=0)


@pytest.mark.parametrize("shape,axis", [((5, 12), 1), ((5, 12), -1), ((5, 12), 0), ((3, 7, 10), 2), ((3, 7, 10), -1),
                                        ((3, 7, 10), 1), ((3, 7, 10), -2), ((3, 7, 10), -3)])
@pytest.mark.parametrize("p", [1, 2])
def test_lp_normalization(native, tmp_path, shape, axis, p):
    from die_amd.utils.onnx_writer import GraphBuilder

    x = np.random.default_rng(len(shape) * 10 + p).standard_normal(shape).astype(np.float32)
    g = GraphBuilder(name="lpn")
    y = g.node("LpNormalization", [g.input("x", ["N"] + list(shape[1:]))], name="normalize", axis=axis, p=p)
    g.output(y, ["N"] + list(shape[1:]))
    x64 = x.astype(np.float64)
    nrm = np.abs(x64).sum(axis=axis, keepdims=True) if p == 1 else np.sqrt((x64 ** 2).sum(axis=axis, keepdims=True))
    got = _run(native, tmp_path, g, x, "lpn")
    assert got.shape == x.shape
    np.testing.assert_allclose(got, x64 / nrm, rtol=3e-6, atol=0)


def test_lp_normalization_has_no_epsilon(native, tmp_path):
    """ONNX: an all-zero row is 0 / 0 = NaN; its neighbours are untouched."""
    from die_amd.utils.onnx_writer import GraphBuilder

    g = GraphBuilder(name="lpn0")
    g.output(g.node("LpNormalization", [g.input("x", ["N", 4])], name="normalize", axis=-1, p=2), ["N", 4])
    x = np.array([[0, 0, 0, 0], [3, 0, 4, 0]], np.float32)
    got = _run(native, tmp_path, g, x, "lpn0")
    assert np.isnan(got[0]).all()
    np.testing.assert_allclose(got[1], [0.6, 0, 0.8, 0], rtol=1e-6)


def _pooling_tail(expanded):
    """rows [N, S * D] + a 0 / 1 mask in the last S columns of the same input -> the sbert_ids tail
    (expanded mask, [N, D] count, F.normalize) or the sbert_ids_hf one ([N, S, 1] mask, [N, 1] count,
    LpNormalization)."""
    from die_amd.utils.onnx_writer import GraphBuilder

    S, D = 6, 10
    g = GraphBuilder(name="pool_tail")
    x = g.input("x", ["N", S * D + S])
    h = g.node("Reshape", [g.node("Slice", [x, g.const(np.array([0], np.int64), "s0"), g.const(np.array([S * D], np.int64), "e0"),
                                            g.const(np.array([1], np.int64), "ax")], name="rows_flat"),
                           g.const(np.array([0, S, D], np.int64), "rows_shape")], name="rows")
    ids = g.node("Slice", [x, g.const(np.array([S * D], np.int64), "s1"), g.const(np.array([S * D + S], np.int64), "e1"),
                           g.const(np.array([1], np.int64), "ax1")], name="ids")
    vis = g.node("Greater", [ids, g.const(np.array(0, np.float32), "pad")], name="visible")
    last = g.const(np.array([-1], np.int64), "last_axis")
    tokens = g.const(np.array([1], np.int64), "token_axis")
    cmin = g.const(np.array(1e-9, np.float32), "count_min")
    if expanded:
        m = g.node("Cast", [g.node("Expand", [g.node("Unsqueeze", [vis, last], name="pool_mask"),
                                              g.node("Shape", [h], name="states_shape")], name="pool_mask_expanded")],
                   name="pool_mask_f", to=1)
        summed = g.node("ReduceSum", [g.node("Mul", [h, m], name="masked_states"), tokens], name="masked_sum", keepdims=0)
        count = g.node("Clip", [g.node("ReduceSum", [m, tokens], name="visible_count", keepdims=0), cmin], name="count_clamp")
        pooled = g.node("Div", [summed, count], name="mean_pool")
        norm = g.node("Clip", [g.node("ReduceL2", [pooled], name="norm", axes=[-1], keepdims=1),
                               g.const(np.array(1e-12, np.float32), "norm_eps")], name="norm_clamp")
        y = g.node("Div", [pooled, g.node("Expand", [norm, g.node("Shape", [pooled], name="pooled_shape")],
                                          name="norm_expanded")], name="normalize")
    else:
        mf = g.node("Cast", [vis], name="mask_f", to=1)
        summed = g.node("ReduceSum", [g.node("Mul", [g.node("Unsqueeze", [mf, last], name="pool_mask"), h],
                                             name="masked_states"), tokens], name="masked_sum", keepdims=0)
        count = g.node("Max", [g.node("ReduceSum", [mf, tokens], name="visible_count", keepdims=1), cmin], name="count_clamp")
        y = g.node("LpNormalization", [g.node("Div", [summed, count], name="mean_pool")], name="normalize", axis=1, p=2)
    g.output(y, ["N", D])
    return g, S, D


@pytest.mark.parametrize("expanded", [True, False])
def test_pooling_tail_on_padding_a_hole_and_length_one(native, tmp_path, expanded):
    g, S, D = _pooling_tail(expanded)
    rng = np.random.default_rng(3)
    rows = rng.standard_normal((4, S, D)).astype(np.float32)
    vis = np.array([[1, 1, 1, 1, 0, 0],   # padding
                    [1, 1, 0, 1, 1, 0],   # a hole and padding
                    [1, 0, 0, 0, 0, 0],   # length 1
                    [1, 1, 1, 1, 1, 1]], np.float32)
    x = np.concatenate([rows.reshape(4, -1), vis * 7.0], axis=1)  # "ids" 7 = visible, 0 = pad
    got = _run(native, tmp_path, g, x, "tail%d" % expanded)
    r64 = rows.astype(np.float64)
    mean = (r64 * vis[:, :, None]).sum(1) / np.maximum(vis.sum(1, keepdims=True), 1e-9)
    ref = mean / np.maximum(np.linalg.norm(mean, axis=1, keepdims=True), 1e-12)
    assert got.shape == (4, D)
    np.testing.assert_allclose(got, ref, rtol=0, atol=2e-6)
    np.testing.assert_allclose(np.linalg.norm(got.astype(np.float64), axis=1), 1.0, atol=1e-6)
    # length 1: the vector is the first row, normalised
    np.testing.assert_allclose(got[2], r64[2, 0] / np.linalg.norm(r64[2, 0]), atol=2e-6)
