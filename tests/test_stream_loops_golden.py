"""CPU only: the video-stream checker (tests/stream_oracle.py::NodeLoop with its tracker, solver, motion-source and filter plugs)
gives, bit for bit, what the four hand-kept loops it replaced gave - tests/golden/stream_loops.npz, recorded from those loops
(tests/golden/make_golden_stream_loops.py says how).  It tests the reference the GPU stream tests compare against."""
import importlib.util
import os

import numpy as np
import pytest

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


@pytest.fixture(scope="module")
def gen(pkg):
    spec = importlib.util.spec_from_file_location("make_golden_stream_loops", os.path.join(GOLDEN, "make_golden_stream_loops.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture(scope="module")
def pinned():
    with np.load(os.path.join(GOLDEN, "stream_loops.npz")) as z:
        return {k: z[k] for k in z.files}


def per_step(arrays, case, field):
    return np.split(arrays[f"{case}/{field}"], np.cumsum(arrays[f"{case}/{field}.size"])[:-1])


@pytest.mark.parametrize("group", ["plain", "seeded", "node", "robust"])
def test_the_loop_gives_the_recorded_outputs(gen, pinned, group):
    got = gen.record(group)
    cases = sorted({k.split("/")[0] for k in got})
    want = {k: a for k, a in pinned.items() if k.split("/")[0] in cases}
    assert sorted(got) == sorted(want) and len(cases) == {"plain": 2, "seeded": 1, "node": 3, "robust": 6}[group]
    for k in want:                                               # a field that was None in a step has size -1 there: None matches None
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].tobytes() == want[k].tobytes(), k
    # the recording is not vacuous
    redetected = solved = 0
    for case in cases:
        assert want[f"{case}/tracks"].dtype == np.float32 and want[f"{case}/first"].dtype == np.float32
        n_old, n_tracked = want[f"{case}/n_old"], want[f"{case}/n_tracked"]
        redetected += int(np.count_nonzero(want[f"{case}/tracks.size"] // 2 > n_tracked))
        solved += int(np.count_nonzero(want[f"{case}/v.size"] == 3))
        if case.endswith("drop"):
            zero = [int(np.count_nonzero(w == 0)) - int(a - b) for w, a, b in zip(per_step(want, case, "weights"), n_old, n_tracked)]
            assert max(zero) > 0, (case, zero)                   # tracked points (status 1) whose final weight is 0: what `drop` removes
    assert redetected > 0 and solved > 0
    if group == "robust":
        assert sum(c.endswith("drop") for c in cases) == 3
