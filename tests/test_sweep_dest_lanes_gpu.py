"""GPU parity of the destination-lane chunk loop (OPT_SWEEP_LANES 1, k_sweep_dest_lanes): a wave
tests 8 sources x 64 consecutive destinations instead of 64 sources x 8 destinations, and logs
its hits in the source-lane loop's format for the unchanged exact pass.

Every case computes at least four times on one engine with OPT_SWEEP_LANES 1 and 0 alternating
(the first computation runs in grid order, the later ones heavy-first, and each shape's order
buffer meets the other shape's launch) and compares every computation with the CPU oracle bit for
bit: kind, latency, hops and reliability.
"""
import functools

import numpy as np
import pytest

from paritylib import assert_bitexact, oracle_matrix
from shadow_amd import engine as E
from shadow_amd import synth

pytestmark = pytest.mark.gpu

LANES = (1, 0, 1, 0, 1)


def _graph(case):
    if case == "partial_tile":
        # 611 = 9 * 64 + 35: the last destination tile is partial; 150 sources = 3 batches, the last
        # with 22: two full octets, a partial one, an empty one, and the upper half of its lanes empty
        return synth.geometric_complete_ish(V=611, A=150)
    if case == "one_batch_parts":
        return synth.geometric_complete_ish(V=900, A=70)  # batches of 64 and 6: one per part
    if case == "ties":
        return synth.integer_grid(rows=14, cols=15, seed=6)  # taint and replayed sources
    if case == "directed":
        return synth.random_sparse(V=300, avg_deg=40, seed=9, directed=True)  # W is asymmetric
    if case == "vloss_prefer":
        g = synth.geometric_complete_ish(V=600, A=200)
        rng = np.random.default_rng(3)
        g.vertex_packetloss = np.where(rng.random(g.n) < 0.3, rng.uniform(0, 0.05, g.n), np.nan)
        g.prefer_direct = True
        return g
    raise AssertionError(case)


def _oracle(g):
    olat, orel, ohops, okind, og = oracle_matrix(g)
    og.close()
    return olat, orel, ohops, okind


@functools.lru_cache(maxsize=None)
def _oracle_of_case(case):  # computed once per case, shared by the tests that use it, never written
    return _oracle(_graph(case))


def _check(eng, want, tag):
    olat, orel, ohops, okind = want
    for step, lanes in enumerate(LANES):
        eng.set_option(E.OPT_SWEEP_LANES, lanes)
        lat, rel, hops, kind = eng.compute_rows()
        for name, x, y in (("kind", kind, okind), ("latency", lat, olat), ("hops", hops, ohops),
                           ("reliability", rel, orel)):
            assert_bitexact(f"{tag} step {step} lanes {lanes} {name}", x, y)


@pytest.mark.parametrize("case", ["partial_tile", "one_batch_parts", "ties", "directed", "vloss_prefer"])
def test_dest_lanes_matches_oracle(case):
    g = _graph(case)
    want = _oracle_of_case(case)
    eng = E.Engine.from_synth(g, layout="dense")
    eng.set_attached(g.attached)
    _check(eng, want, case)
    eng.close()


@pytest.mark.parametrize("mode", ["full_sweeps", "host_rounds"])
def test_dest_lanes_round_modes(mode):
    """every round a full sweep (OPT_DELTA_PERMILLE 0: the later sweeps are unseeded and take their
    thresholds from the current distances), and host-driven rounds (OPT_DENSE_SPEC 0)"""
    g = _graph("partial_tile")
    want = _oracle_of_case("partial_tile")
    eng = E.Engine.from_synth(g, layout="dense")
    if mode == "full_sweeps":
        eng.set_option(E.OPT_DELTA_PERMILLE, 0)
    else:
        eng.set_option(E.OPT_DENSE_SPEC, 0)
    eng.set_attached(g.attached)
    _check(eng, want, mode)
    eng.close()


def test_dest_lanes_second_attached_set():
    """a second attached set between computations: other sources, the same order buffers"""
    g = _graph("partial_tile")
    other = np.sort(np.random.default_rng(21).choice(g.n, size=len(g.attached), replace=False)).astype(np.int32)
    eng = E.Engine.from_synth(g, layout="dense")
    for k, att in enumerate((g.attached, other, g.attached)):
        g.attached = att
        want = _oracle(g) if k == 1 else _oracle_of_case("partial_tile")
        eng.set_attached(att)
        _check(eng, want, f"set {k}")
    eng.close()
