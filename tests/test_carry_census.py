"""The host side of mg_carry_census on the CPU: the start
rule ``carry.starts_ref`` against a brute-force recount of random verdict bits,
mg_carry_starts_host against ``starts_ref``, the plan of the device buffer
against the ladder's, their refusals, and the miss report."""

import numpy as np
import pytest

from mythril_amd import carry as CY
from mythril_amd import census as CS
from mythril_amd import engine as E
from mythril_amd.engine import EngineError
from mythril_amd.smt import node as N


def verdicts(seed, n_roots, n_rungs, lanes, style):
    """(n_rungs * lanes, n_roots) bool.  ``style``: "sparse" nearly all true
    (hits, many sole columns), "stuck" one root false everywhere (no hit, no
    sole column unless the others hold), "rung1" one root false on every rung
    but rung 1, "noise" fair coins (with many roots: no sole column at all)."""
    rng = np.random.default_rng(seed)
    n = n_rungs * lanes
    if style == "noise":
        return rng.random((n, n_roots)) < 0.5
    bits = rng.random((n, n_roots)) < (0.98 if style == "sparse" else 0.9)
    k = int(rng.integers(n_roots))
    if style == "stuck":
        bits[:, k] = False
    if style == "rung1":
        bits[:, k] = False
        bits[lanes:2 * lanes, :] = True
    return bits


def censuses_of(bits, n_rungs, lanes):
    return [CS.reduce_bits(bits[r * lanes:(r + 1) * lanes], r * lanes) for r in range(n_rungs)]


def brute_starts(bits, n_rungs, lanes, walkers):
    """The rule from the bits alone, column by column."""
    nfail = (~bits).sum(axis=1)
    bests = []
    for r in range(n_rungs):
        cols = range(r * lanes, (r + 1) * lanes)
        bests.append(min(cols, key=lambda c: (nfail[c], c)))
    lst = [(b, int(nfail[b])) for _, b in sorted(enumerate(bests),
                                                 key=lambda rb: (nfail[rb[1]], rb[0]))]
    for r in range(n_rungs):
        for k in range(bits.shape[1]):
            for c in range(r * lanes, (r + 1) * lanes):
                if nfail[c] == 1 and not bits[c, k]:
                    if c != bests[r]:
                        lst.append((c, 1))
                    break
    n = len(lst)
    assert len({c for c, _ in lst}) == n                    # no column twice before the padding
    lst = (lst + [lst[0]] * walkers)[:walkers]
    return [c for c, _ in lst], [f for _, f in lst], n


CASES = [(n_roots, n_rungs, lanes, style)
         for n_roots in (3, 33, 257)
         for n_rungs, lanes, style in ((1, 1, "sparse"), (2, 63, "rung1"), (3, 256, "sparse"),
                                       (5, 63, "stuck"), (8, 63, "noise"), (8, 256, "sparse"),
                                       (4, 1, "noise"), (6, 256, "rung1"), (7, 63, "sparse"))]


@pytest.mark.parametrize("n_roots,n_rungs,lanes,style", CASES)
def test_starts_ref_and_the_host_export_equal_a_brute_force_recount(n_roots, n_rungs, lanes, style):
    bits = verdicts(n_roots * 1000 + n_rungs * 10 + lanes, n_roots, n_rungs, lanes, style)
    cs = censuses_of(bits, n_rungs, lanes)
    blocks = np.stack([CS.pack_block(c) for c in cs])
    for c, b in zip(cs, blocks):
        c.check()
        assert CS.unpack_block(b, n_roots, c.first_index, lanes) == c
    for walkers in (1, 4, 64):
        want_col, want_nfail, n = brute_starts(bits, n_rungs, lanes, walkers)
        col, nfail = CY.starts_ref(cs, walkers)
        assert col.dtype == np.int64 and nfail.dtype == np.uint32
        assert col.tolist() == want_col and nfail.tolist() == want_nfail
        hcol, hnfail = E.carry_starts_host(blocks, n_roots, walkers)
        assert hcol.tolist() == want_col and hnfail.tolist() == want_nfail
        if style == "rung1":
            # a hit on rung 1 only: start 0 is its lowest column
            assert (col[0], nfail[0]) == (lanes, 0)
        if style == "stuck":
            assert nfail[0] >= 1


def test_the_inputs_cover_padding_a_longer_list_and_no_sole_column():
    seen = set()
    for n_roots, n_rungs, lanes, style in CASES:
        bits = verdicts(n_roots * 1000 + n_rungs * 10 + lanes, n_roots, n_rungs, lanes, style)
        cs = censuses_of(bits, n_rungs, lanes)
        n_sole = sum(int((c.sole_index >= 0).sum()) for c in cs)
        for walkers in (1, 4, 64):
            n = brute_starts(bits, n_rungs, lanes, walkers)[2]
            seen.add("padding" if n < walkers else "longer" if n > walkers else "exact")
        if n_sole == 0:
            seen.add("no sole column")
        if n_sole > 64:
            seen.add("more than W sole columns")
    assert {"padding", "longer", "no sole column", "more than W sole columns"} <= seen


def test_starts_of_nothing_and_the_host_refusals():
    col, nfail = CY.starts_ref([CS.reduce_bits(np.zeros((0, 3), dtype=bool), 0)], 2)
    assert col.tolist() == [-1, -1] and nfail.tolist() == [0xFFFFFFFF] * 2
    empty = CS.pack_block(CS.reduce_bits(np.zeros((0, 3), dtype=bool), 0))[None, :]
    hcol, hnfail = E.carry_starts_host(empty, 3, 2)
    assert hcol.tolist() == [-1, -1] and hnfail.tolist() == [0xFFFFFFFF] * 2
    ok = np.zeros((1, 17), dtype=np.uint64)
    for blocks, n_roots, walkers in ((ok, 3, 0), (ok, 3, 65), (np.zeros((9, 17), np.uint64), 3, 1),
                                     (np.zeros((0, 17), np.uint64), 3, 1),
                                     (np.zeros((1, 2), np.uint64), 0, 1),
                                     (np.zeros((1, 5 * 1025 + 2), np.uint64), 1025, 1)):
        with pytest.raises(EngineError):
            E.carry_starts_host(blocks, n_roots, walkers)
    with pytest.raises(ValueError):
        E.carry_starts_host(np.zeros((1, 16), dtype=np.uint64), 3, 1)


def test_census_plan_is_the_ladders_plan_with_counters_and_probes_added():
    n_leaves, n_rungs = [3, 274, 15, 0], [3, 1, 2, 8]
    n_roots, n_probes, probe0 = [5, 257, 1024, 1], [1, 3, 4, 2], [0, 1, 0, 1]
    for lanes, walkers, max_leaves in ((1, 1, 274), (63, 4, 300), (256, 64, 274)):
        off, total, leaf_w, probe_w = E.carry_census_plan_host(
            n_leaves, n_rungs, n_roots, n_probes, probe0, lanes, walkers, max_leaves)
        lad, lad_total, lad_leaf_w = E.carry_ladder_plan_host(n_leaves, n_rungs, lanes, max_leaves)
        n, cols = 4, 8 * lanes
        base = E.CARRY_SHARED + n * E.CARRY_JOB_REGIONS
        assert len(off) == base + E.CARRY_CENSUS_SHARED + n * E.CARRY_CENSUS_JOB_REGIONS
        assert not (off % 256).any() and total % 256 == 0
        # the uploaded front lies where the ladder has it; the census records
        # begin where the ladder's output block would
        assert off[:3].tolist() == lad[:3].tolist() and leaf_w == lad_leaf_w
        for g in range(n):
            at = E.CARRY_SHARED + g * E.CARRY_JOB_REGIONS
            assert off[at:at + 3].tolist() == lad[at:at + 3].tolist()
        assert off[base] == lad[3]
        r256 = lambda b: (b + 255) // 256 * 256                       # noqa: E731
        at = int(off[base]) + r256(n * 24)
        for g in range(n):
            assert off[base + 1 + 2 * g] == at
            at += r256((5 * n_roots[g] + 2) * 8 * n_rungs[g])
        # counters, then the output block: one download; then leaves and probes
        assert off[3] == at
        at += r256(n * walkers * (12 + max_leaves * 32))
        for g in range(n):
            assert off[E.CARRY_SHARED + g * E.CARRY_JOB_REGIONS + 3] == at
            at += leaf_w * 4
        assert probe_w * 4 == r256(max(n_probes) * 32 * cols)
        for g in range(n):
            assert off[base + 2 + 2 * g] == at
            at += probe_w * 4
        assert at == total
        # without the counters, the census records, the wider output block and
        # the probe regions it is the ladder's size
        extra = r256(n * 24) + sum(r256((5 * r + 2) * 8 * k) for r, k in zip(n_roots, n_rungs)) + \
            r256(n * walkers * (12 + max_leaves * 32)) - r256(n * (16 + max_leaves * 32)) + \
            n * probe_w * 4
        assert total - extra == lad_total


def test_census_plan_refusals():
    good = dict(n_leaves=[3, 4], n_rungs=[2, 3], n_roots=[5, 300], n_probes=[1, 2],
                mask_probe0=[0, 0], lanes=64, walkers=4, max_leaves=4)
    E.carry_census_plan_host(**good)
    for change in ({"walkers": 0}, {"walkers": 65}, {"n_roots": [0, 300]}, {"n_roots": [5, 1025]},
                   {"n_probes": [1, 1]}, {"mask_probe0": [1, 0]}, {"mask_probe0": [0, 1]},
                   {"n_rungs": [0, 3]}, {"n_rungs": [2, 9]}, {"lanes": 0},
                   {"lanes": (1 << 20) // 3 + 1}, {"n_leaves": [], "n_rungs": [], "n_roots": [],
                                                    "n_probes": [], "mask_probe0": []}):
        with pytest.raises(EngineError, match="carry_census"):
            E.carry_census_plan_host(**dict(good, **change))
    with pytest.raises(ValueError):
        E.carry_census_plan_host(**dict(good, n_roots=[5]))
    big = dict(n_leaves=[0xFFFFFFFF] * 256, n_rungs=[8] * 256, n_roots=[1024] * 256,
               n_probes=[4] * 256, mask_probe0=[0] * 256, lanes=1 << 17, walkers=64, max_leaves=1)
    with pytest.raises(EngineError):
        E.carry_census_plan_host(**big)


def test_exports_and_the_knobs_defaults():
    lib = E.load_library(check_digest=False)
    for name in ("mg_carry_census", "mg_carry_census_plan_host", "mg_carry_starts_host"):
        assert name in E.EXPORTS and getattr(lib, name)
    assert CY.MAX_WALKERS == E.CARRY_MAX_WALKERS == 64 and CY.CARRY_WALKERS == 4


def test_compile_census_ck_is_the_ck_eval_form_with_the_mask_probes():
    from mythril_amd.assign import Assignment
    x, y = N.bv_var("ccx", 16), N.bv_var("ccy", 16)
    nodes = [N.bv_cmp("bvult", x, N.bv_num(100, 16)), N.distinct(x, y)]
    asg = Assignment()
    asg.vars["ccx"] = 7
    probes = CS.mask_probes(nodes)
    prog = CY.compile_census_ck(nodes, asg, probes)
    plain = CY.compile_eval_ck(nodes, asg)
    assert prog is CY.compile_census_ck(nodes, asg, probes)            # cached
    assert prog is not plain and prog.n_probes == 1 and plain.n_probes == 0
    assert [(l.name, l.width) for l in prog.leaves] == [(l.name, l.width) for l in plain.leaves]


def test_miss_report_lists_the_blockers_of_every_kept_rung():
    x, y = N.bv_var("mrx", 16), N.bv_var("mry", 16)
    nodes = [N.bv_cmp("bvult", x, N.bv_num(100, 16)), N.distinct(x, y),
             N.bv_cmp("bvult", y, N.bv_num(5, 16))]
    bits = np.ones((8, 3), dtype=bool)
    bits[:, 2] = False                     # root 2 never holds
    bits[1, 0] = False
    cs = [CS.reduce_bits(bits[:4], 0), CS.reduce_bits(bits[4:], 4)]
    rep = CY.miss_report(nodes, cs, [0, 2])
    assert [r["rung"] for r in rep] == ["all", "new"]
    assert [b["root"] for b in rep[0]["blockers"]] == [2, 0]
    assert rep[0]["blockers"][0] == {"root": 2, "constraint": repr(nodes[2]), "pass": 0,
                                     "first_block": 3, "sole_block": 3}
    assert [b["root"] for b in rep[1]["blockers"]] == [2] and rep[1]["best_nfail"] == 1


# ---------------------------------------------------------------------------
# _repair_steps without ``carried`` runs as it always has
# ---------------------------------------------------------------------------

class _StubEngine:
    """Records every call ``repair_group`` makes and answers from canned
    data: a census whose best candidate fails roots, rows that name their
    candidate, a walk that ends with nothing failing."""

    def __init__(self, n_roots):
        self.calls, self.n_roots = [], n_roots

    def load(self, program, leafgen=None, prog_seed=0):
        self.calls.append(("load", program.n_probes, len(program.leaves), len(list(leafgen)),
                           prog_seed))
        return type("Loaded", (), {"program": program})()

    def census(self, lp, seed, first, n_cand, n_roots, mask_probe0=0, chunk=0):
        self.calls.append(("census", seed, first, n_cand, n_roots, mask_probe0))
        rng = np.random.default_rng(5)
        bits = rng.random((64, n_roots)) < 0.8
        bits[:, 0] = False                                    # no candidate is a model ...
        bits[7, 1:] = True                                    # candidates 7 and 9: only root 0
        bits[9, 1:] = True
        bits[11] = True
        bits[11, 2] = False                                   # candidate 11: only root 2
        return CS.reduce_bits(bits, first)

    def witness(self, lp, seed, index):
        self.calls.append(("witness", seed, index))
        rows = np.zeros((len(lp.program.leaves), 8), dtype=np.uint32)
        rows[:, 0] = index
        return rows, None

    def _walk(self, name, lp, starts, n_roots, *rest):
        from mythril_amd.repair import WalkResult
        self.calls.append((name, np.asarray(starts)[:, 0, 0].tolist(), n_roots, rest[-4:]))
        w = starts.shape[0]
        return WalkResult(np.array(starts, copy=True), np.zeros(w, dtype=np.uint32),
                          np.zeros(w, dtype=np.uint64), 3, np.zeros((w, 8, 2), dtype=np.uint32), 1)

    def __getattr__(self, name):
        if name.startswith("walk"):
            return lambda *a: self._walk(name, *a)
        raise AttributeError(name)

    def eval(self, lp, leaves_soa, want_probes=False):
        self.calls.append(("eval", leaves_soa.shape, int(leaves_soa[0, 0, 0])))
        probes = np.full((lp.program.n_probes, 8, 1), 0xFFFFFFFF, dtype=np.uint32)
        return np.array([True]), probes


def drive_repair_group(RP, monkeypatch_engine):
    """``repair_group`` of the gen_cases "flats" case on the stub: the calls
    and the dict without the objects that have no value semantics."""
    import gen_cases as G
    nodes = G.case("flats")
    eng = _StubEngine(len(nodes))
    monkeypatch_engine(lambda device=0, slot=0, nreg=None: eng)
    out = RP.repair_group(nodes, n_cand=64, form="eval", lanes=128, max_rounds=8, seed=77,
                          sync_every=4, scored="sum", walkers=4)
    flat = {k: v for k, v in out.items()
            if k in ("n_roots", "status", "scoring", "start", "starts")}
    flat["census"] = out["census"].as_dict()
    flat["assignment"] = repr(out["assignment"])
    flat["winner_rows"] = out["repair"].leaves[:, 0, 0].tolist()
    return eng.calls, flat


def test_repair_steps_without_carried_makes_the_calls_and_the_dict_it_always_made(monkeypatch):
    import inspect

    from mythril_amd import repair as RP
    assert inspect.signature(RP._repair_steps).parameters["carried"].default is None
    calls, flat = drive_repair_group(
        RP, lambda fn: monkeypatch.setattr(E, "get_engine", fn))
    names = [c[0] for c in calls]
    # view and full program, the census, one witness per distinct pick, the
    # wide views, ONE walk, the fresh evaluation of the winner
    assert names == ["load", "load", "census", "witness", "witness", "load", "load", "walk_sum",
                     "eval"]
    assert calls[2] == ("census", 0x6D797468, 0, 64, 90, 0)
    # the best candidate, then the sole candidates of the blockers in rank
    # order, padded with the best: 7 fails root 0 alone, 11 root 2 alone
    assert flat["starts"] == [7, 11, 7, 7] and flat["start"] == {"index": 7, "nfail": 1}
    assert [c[2] for c in calls[3:5]] == [7, 11]
    assert calls[7][1] == [7, 11, 7, 7] and calls[7][3] == (77, 128, 8, 4)
    assert flat["status"] == "repaired" and flat["winner_rows"] == [7, 11, 7, 7]
    assert calls[8] == ("eval", (274, 8, 1), 11)                 # the winner is walker 1
