"""GPU: a seeded slice of the randomised Or-opt parity sweep (tools/stress_or_opt.py) under `-m gpu`: 6 seeds x 40 cases --
sizes around the wave / row-group / chunk boundaries, EUC_2D / ATT / CEIL_2D / MAN_2D / MAX_2D, *_ICOORD and general
instances, both cost modes, random / greedy / 2-opt-optimal starts, move caps, batches and the 2-opt + Or-opt composite,
every result against tests/or_opt_ref.py bit for bit."""
import os
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tools"))


@pytest.fixture(scope="module")
def ctx():
    from tsp_optimization_amd import engine as E
    c = E.Context(0)
    yield c
    c.close()


@pytest.mark.parametrize("seed", [4001, 4002, 4003, 4004, 4005, 4006])
def test_randomised_or_opt_slice(ctx, seed):
    import stress_or_opt
    assert stress_or_opt.run(seed, 40, ctx=ctx, verbose=False) == 0
