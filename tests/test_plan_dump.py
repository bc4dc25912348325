"""native.plan_dump: the whole plan as text (the identity check of tools/plan_dump.py).  CPU only."""


def _op_lines(text):
    return [l for l in text.splitlines() if l.startswith("op ")]


def test_dump_is_deterministic(native, models):
    path = models["tiny"][0]
    a = native.plan_dump(path)
    assert a == native.plan_dump(path)
    assert a.splitlines()[-1].startswith("plan ") and "params_fnv1a=" in a


def test_dump_tells_plans_apart(native, models):
    path = models["tiny"][0]
    assert native.plan_dump(path, precision="bf16") != native.plan_dump(path, precision="fp32")
    assert native.plan_dump(path, fuse_pairs=True) != native.plan_dump(path, fuse_pairs=False)


def test_one_line_per_op(native, models):
    for path in (models["tiny"][0], models["get_vit"]("tiny")[0]):
        for precision in ("bf16", "fp32"):
            for kw in ({}, {"fuse_pairs": False}, {"side_branches": True}):
                ops = native.plan_summary(path, precision=precision, **kw)["ops"]
                assert len(_op_lines(native.plan_dump(path, precision=precision, **kw))) == len(ops)
