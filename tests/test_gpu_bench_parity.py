"""Parity over the WHOLE bench configuration, not a sample.

``bench.py`` times ``mg_batch_eval_gen`` over every DAG of a workload (C2:
4096 corpus DAGs; C3 / C4: 256 distinct stand-in queries).  Here the same
entry point runs over every one of them at a 2^12-lane slice from a nonzero
first index, and every root bit and every per-DAG first satisfying index is
compared with ``oracle/evalref.c`` (``run_gen``: the same generator, the same
pools; pinned to ``oracle/smtlib_ref.py`` by tests/test_evalref.py).

The interpreter selects among up to 64 handler variants per opcode from
static properties, so the test also asserts that every
(family, variant) the bench configurations execute — reported by the
translator itself (``engine.handler_variants``) — belongs to a program this
test ran, its root bit (the AND of all its roots) compared on every lane.
That bit is false on almost every lane, so it says little about a single
value: every node value and every root bit of a cover of the same variants
is compared in ``tests/test_gpu_value_parity.py``.

The whole-configuration tests run once per register layout (the ``layout``
fixture) in one process: the default 16 slots, then the four-wave 11-slot
layout that ``bench.py`` runs C2 on (the library's second interpreter, chosen
by the context: ``get_engine(0, nreg=11)``).  Programs are compiled for the
layout's slots and translated for its LDS regions.  The oracle's root bits
are computed once per unit: they depend on its roots, leaves and constant
pool, which ``units`` asserts equal on both layouts, not on its registers.
"""

import ctypes as C
import os

import numpy as np
import pytest

import bench
import gpu_batch as G
from mythril_amd import shard
from mythril_amd.build import LAYOUT_LDS_SLOTS
from mythril_amd.engine import default_leafgen, get_engine, handler_variants

pytestmark = pytest.mark.gpu
N_LANES, FIRST = 1 << 12, (3 << 20) + 192
SEED = bench.SEED
FULL = {w: bench.default_units(w) for w in ("c2", "c3", "c4", "c5")}
UNITS = [(w, d) for w, n in FULL.items() for d in range(n)]
LAYOUTS = (16, 11)
# per layout: (family, variant) handlers of the programs verified lane by lane below
CHECKED = {nreg: set() for nreg in LAYOUTS}
# (root bits, gpu_batch.oracle_inputs) of every unit of UNITS: computed by
# the first layout that needs them, shared with the second
_ORACLE = []


def _every_unit(fn, *tail):
    """``fn((workload, unit) + tail)`` for every bench unit, on spawned
    workers (this process may already hold the GPU).  A worker that dies (an
    abort in the C oracle) raises BrokenProcessPool at once instead of
    hanging the module (round 4)."""
    from mythril_amd.procmap import process_map
    return process_map(fn, [u + tail for u in UNITS], min(16, os.cpu_count() or 1), "spawn",
                       chunksize=8)


@pytest.fixture(scope="module", params=LAYOUTS, ids=lambda nreg: "%dslot" % nreg)
def layout(request):
    """(register slots, their context, their LDS spill regions): every test
    of one layout runs, and its programs and images are dropped, before the
    next layout's are built."""
    nreg = request.param
    return nreg, get_engine(0, nreg=nreg), LAYOUT_LDS_SLOTS[nreg]


def test_layout_of_this_context(layout):
    """The context, the compiler and the translator agree on one layout."""
    from mythril_amd import asmgen
    nreg, engine, lds = layout
    assert engine.nreg == nreg and engine.lds_slots == lds
    with asmgen.layout(nreg):
        assert engine.lib.mg_asm_digest_layout(nreg).decode() == asmgen.digest()
    _, p, _, _ = bench.compile_unit(("c2", 0, nreg))
    assert p.nreg == nreg
    print("layout: %d slots, %d LDS regions, %s" % (nreg, lds,
                                                     os.path.basename(bench.engine_lib_path())))


@pytest.fixture(scope="module")
def units(layout):
    """Per workload, every bench unit as (unit, its program on this layout,
    its oracle root bits)."""
    nreg = layout[0]
    if not _ORACLE:
        _ORACLE.extend(_every_unit(G.oracle_root_bits, FIRST, N_LANES))
    out = {w: [] for w in FULL}
    for (w, d), (_, p, _, _), (want, inputs) in zip(UNITS, _every_unit(bench.compile_unit, nreg),
                                                    _ORACLE):
        # never loosen: the shared bits are the oracle's for this program
        # only while it reads the same leaves and the same constant pool
        assert p.nreg == nreg and G.oracle_inputs(p) == inputs, (w, d, nreg)
        out[w].append((d, p, want))
    return out


@pytest.fixture(scope="module")
def images(layout, units):
    """Compiled-program code objects of every bench unit (bench.py --jit),
    built on spawned workers."""
    from mythril_amd import jit
    return {w: jit.compile_batch([(p, None, d) for d, p, _ in units[w]], workers=16,
                                 start="spawn", lds_slots=layout[2]) for w in FULL}


@pytest.mark.parametrize("path", ["interp", "jit"])
@pytest.mark.parametrize("workload", ["c2", "c3", "c4", "c5"])
def test_every_bench_unit_every_lane(layout, units, images, workload, path):
    nreg, engine, lds = layout
    us = units[workload]
    assert [d for d, _, _ in us] == list(range(FULL[workload]))
    bits, firsts = G.run_batch(engine, [(d, p) for d, p, _ in us], SEED, FIRST, N_LANES,
                               images[workload] if path == "jit" else None)
    n_hit, n_sat = G.assert_matches_oracle(bits, firsts, [want for _, _, want in us], FIRST,
                                           (workload, path, nreg))
    if path == "interp":
        for d, p, _ in us:
            CHECKED[nreg].update(handler_variants(p, lds))
    print("%s %s: %d units, %d with satisfying lanes, %d satisfying lanes (%d-slot layout)"
          % (workload, path, len(us), n_hit, n_sat, nreg))


def test_bench_handler_variants_all_checked(layout, units):
    """Every (family, variant) executed by a bench configuration (what
    bench.py compiles for C2, C3, C4 and C5) belongs to a program the test above
    verified lane by lane; the count is reported so a new variant shows up
    in the log."""
    nreg, _, lds = layout
    assert CHECKED[nreg], "run with test_every_bench_unit_every_lane (same module)"
    bench_set = set()
    for w in FULL:                      # the programs bench.compile_unit builds
        for d, p, _ in units[w]:
            bench_set |= handler_variants(p, lds)
    missing = sorted(bench_set - CHECKED[nreg])
    assert not missing, missing
    fams = sorted({f for f, _ in bench_set})
    print("bench configurations execute %d (family, variant) handlers in %d families "
          "(%d-slot layout)" % (len(bench_set), len(fams), nreg))


def test_jit_attach_refuses_code_compiled_for_other_records(engine):
    """mg_jit_attach compares each table row's record fingerprint with the
    loaded program's: an image compiled for another program (or another
    allocation of the same DAG) is refused, never entered."""
    from mythril_amd import jit
    from mythril_amd.engine import EngineError
    d1, p1, _, _ = bench.compile_unit(("c2", 1))
    d2, p2, _, _ = bench.compile_unit(("c2", 2))
    image = jit.compile_batch([(p1, None, d1)])
    lp2 = engine.load(p2, default_leafgen(p2), prog_seed=d2)
    with pytest.raises(EngineError, match="other records"):
        engine.jit_attach([lp2], image)
    lp1 = engine.load(p1, default_leafgen(p1), prog_seed=d1 + 1)     # another salt
    with pytest.raises(EngineError, match="other records"):
        engine.jit_attach([lp1], image)
    lp1 = engine.load(p1, default_leafgen(p1), prog_seed=d1)
    engine.jit_detach(engine.jit_attach([lp1], image))


def test_program_freed_while_attached_leaves_its_image(engine):
    """A program freed before its image is detached drops out of the image's
    list (mg_free_program), so the detach cannot write into the device block
    the next program reuses: that program keeps evaluating like the
    interpreter did before the detach."""
    from mythril_amd import jit
    d1, p1, _, _ = bench.compile_unit(("c2", 1))
    d2, p2, _, _ = bench.compile_unit(("c2", 2))
    image = jit.compile_batch([(p1, None, d1)])
    lp1 = engine.load(p1, default_leafgen(p1), prog_seed=d1)
    h = engine.jit_attach([lp1], image)
    del lp1                                       # freed while attached
    lp2 = engine.load(p2, default_leafgen(p2), prog_seed=d2)
    before = engine.eval_gen(lp2, bench.SEED, 5, 4096, want_probes=True)
    engine.jit_detach(h)
    after = engine.eval_gen(lp2, bench.SEED, 5, 4096, want_probes=True)
    assert np.array_equal(before[0], after[0])
    assert (before[1] is None and after[1] is None) or np.array_equal(before[1], after[1])


def test_jit_attach_refuses_an_opcode_twin(engine):
    """programs whose records differ only in an operation (ADD vs
    XOR, the handler id in word 0) must not share a fingerprint: the image of
    one is refused for the other, and accepted for itself."""
    from mythril_amd import jit
    from mythril_amd.engine import EngineError
    from test_jit import opcode_twins
    p_add, p_xor = opcode_twins()
    image = jit.compile_batch([(p_add, None, 1)])
    with pytest.raises(EngineError, match="other records"):
        engine.jit_attach([engine.load(p_xor, default_leafgen(p_xor), prog_seed=1)], image)
    lp = engine.load(p_add, default_leafgen(p_add), prog_seed=1)
    engine.jit_detach(engine.jit_attach([lp], image))


def test_jit_attach_refuses_another_interpreter_and_stray_entries(engine, monkeypatch):
    """The table header carries the asm digest of the interpreter the code
    was generated for (pinned registers, descriptor layout): an image made
    for another one is refused.  An entry pointing outside the image's
    executable sections (here: into the table itself) is refused too."""
    from mythril_amd import jit
    from mythril_amd.engine import EngineError
    d1, p1, _, _ = bench.compile_unit(("c2", 1))
    lp = engine.load(p1, default_leafgen(p1), prog_seed=d1)
    real = jit.table_asm
    monkeypatch.setattr(jit.G, "digest", lambda *a: "0123456789abcdef")
    stale = jit.compile_batch([(p1, None, d1)])
    monkeypatch.undo()
    with pytest.raises(EngineError, match="another interpreter"):
        engine.jit_attach([lp], stale)

    def stray(fps, nreg=None):
        return real(fps, nreg).replace("\t.quad mg_jp0 - . + 16\n", "\t.quad 16\n")
    monkeypatch.setattr(jit, "table_asm", stray)
    bad = jit.compile_batch([(p1, None, d1)])
    monkeypatch.undo()
    with pytest.raises(EngineError, match="outside the code"):
        engine.jit_attach([lp], bad)
    engine.jit_detach(engine.jit_attach([lp], jit.compile_batch([(p1, None, d1)])))


def test_free_waits_for_launches_on_every_caller_stream(engine):
    """a long batch queued on caller stream A, then a short one on
    stream B; the first batch and its programs are freed at once and new
    programs are loaded into the recycled device blocks.  The free must wait
    for A too (not only the last stream), so A's results equal a clean run."""
    hip = G.hip()
    ids_a, ids_b, ids_c = range(0, 48), range(48, 50), range(100, 148)
    progs = {d: bench.compile_unit(("c2", d))[1] for d in list(ids_a) + list(ids_b) + list(ids_c)}
    n = 1 << 17
    words = n // 64

    def run_on(stream, ids, d_bits, d_first, free_after=False):
        loaded = [engine.load(progs[d], default_leafgen(progs[d]), prog_seed=d) for d in ids]
        batch = engine.batch_create(loaded)
        engine.batch_eval_gen(batch, SEED, 7, n, d_bits, d_first, stream)
        return loaded, batch

    sa, sb = C.c_void_p(), C.c_void_p()
    assert hip.hipStreamCreate(C.byref(sa)) == 0 and hip.hipStreamCreate(C.byref(sb)) == 0
    dev = G.device_buffer
    try:
        with dev(len(ids_a) * words * 8) as bits_a, dev(len(ids_a) * 8) as first_a, \
                dev(len(ids_b) * words * 8) as bits_b, dev(len(ids_b) * 8) as first_b:
            ones = np.full(len(ids_a), shard.NONE, dtype=np.int64)
            # reference: the same batch alone, completed
            assert hip.hipMemcpy(first_a, ones.ctypes.data_as(C.c_void_p), C.c_size_t(ones.nbytes), 1) == 0
            la, ba = run_on(sa.value, ids_a, bits_a.value, first_a.value)
            assert hip.hipStreamSynchronize(sa) == 0
            want = np.zeros((len(ids_a), words), dtype=np.uint64)
            assert hip.hipMemcpy(want.ctypes.data_as(C.c_void_p), bits_a, C.c_size_t(want.nbytes), 2) == 0
            engine.batch_free(ba)
            del la
            # the race: A long, B short, free A's blocks, reuse them at once
            assert hip.hipMemsetAsync(bits_a, 0, C.c_size_t(want.nbytes), sa) == 0
            la, ba = run_on(sa.value, ids_a, bits_a.value, first_a.value)
            lb, bb = run_on(sb.value, ids_b, bits_b.value, first_b.value)
            engine.batch_free(ba)
            del la
            lc = [engine.load(progs[d], default_leafgen(progs[d]), prog_seed=d) for d in ids_c]
            assert hip.hipDeviceSynchronize() == 0
            got = np.zeros_like(want)
            assert hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), bits_a, C.c_size_t(got.nbytes), 2) == 0
            assert np.array_equal(got, want)
            engine.batch_free(bb)
            del lb, lc
    finally:
        hip.hipStreamDestroy(sa)
        hip.hipStreamDestroy(sb)
