"""What the GPU parity tests (and tools/jit_check.py) share to run a batch
through ``mg_batch_eval_gen`` into raw device buffers and to compare it with
``oracle/evalref.c``: the HIP runtime handle, a device buffer, the batch run,
the oracle worker and the one bit-exact comparison.  A plain module, imported
like ``value_units.py``."""

import contextlib
import ctypes as C
import functools

import numpy as np

import bench
from mythril_amd import shard
from mythril_amd.engine import default_leafgen


@functools.lru_cache(maxsize=None)
def hip():
    """The HIP runtime the library itself uses (torch bundles another one)."""
    return C.CDLL("libamdhip64.so.7")


@contextlib.contextmanager
def device_buffer(nbytes):
    """A device buffer of ``nbytes`` (a ``c_void_p``), freed on exit."""
    p = C.c_void_p()
    assert hip().hipMalloc(C.byref(p), C.c_size_t(nbytes)) == 0
    try:
        yield p
    finally:
        hip().hipFree(p)


def _copy(dst, src, nbytes, kind):
    assert hip().hipMemcpy(dst, src, C.c_size_t(nbytes), kind) == 0


def run_loaded(engine, loaded, seed, first, n, stream=None):
    """One ``batch_eval_gen`` of the loaded programs (their image, if any,
    already attached) over candidates [first, first + n): ``(bits, firsts)``,
    the root bits as a (programs, n) bool array and the first satisfying
    index of each program (``shard.NONE`` when it has none)."""
    assert n % 64 == 0
    bits = np.zeros((len(loaded), n // 64), dtype=np.uint64)
    firsts = np.full(len(loaded), shard.NONE, dtype=np.int64)
    batch = engine.batch_create(loaded)
    try:
        with device_buffer(bits.nbytes) as d_bits, device_buffer(firsts.nbytes) as d_first:
            _copy(d_first, firsts.ctypes.data_as(C.c_void_p), firsts.nbytes, 1)
            engine.batch_eval_gen(batch, seed, first, n, d_bits.value, d_first.value, stream or 0)
            assert hip().hipDeviceSynchronize() == 0
            _copy(bits.ctypes.data_as(C.c_void_p), d_bits, bits.nbytes, 2)
            _copy(firsts.ctypes.data_as(C.c_void_p), d_first, firsts.nbytes, 2)
    finally:
        engine.batch_free(batch)
    return (np.unpackbits(bits.view(np.uint8), axis=1, bitorder="little").astype(bool),
            firsts.tolist())


def run_batch(engine, items, seed, first, n, image=None):
    """``run_loaded`` of ``items = [(prog_seed, Program)]`` loaded with their
    default leaf generators, on their compiled code when ``image``
    (``jit.compile_batch`` of the same items) is given."""
    loaded = [engine.load(p, default_leafgen(p), prog_seed=d) for d, p in items]
    handle = engine.jit_attach(loaded, image) if image is not None else None
    try:
        return run_loaded(engine, loaded, seed, first, n)
    finally:
        if handle is not None:
            engine.jit_detach(handle)


def assert_matches_oracle(bits, firsts, want, first, where, ids=None):
    """Every lane of every unit equals the oracle's root bits ``want`` (one
    bool array per unit), and every first index is ``first`` + the first true
    oracle lane, or ``shard.NONE``.  ``ids`` names the units in a message
    (default: their positions).  Returns (units with satisfying lanes,
    satisfying lanes)."""
    assert len(bits) == len(firsts) == len(want), (where, len(bits), len(firsts), len(want))
    n_hit = n_sat = 0
    for k, w in enumerate(want):
        unit = k if ids is None else ids[k]
        w = np.asarray(w, dtype=bool)
        got = np.asarray(bits[k], dtype=bool)
        assert np.array_equal(got, w), (where, unit, int(np.argmax(got != w)))
        hit = np.flatnonzero(w)
        assert firsts[k] == (first + int(hit[0]) if hit.size else shard.NONE), (where, unit)
        n_hit += bool(hit.size)
        n_sat += int(hit.size)
    return n_hit, n_sat


def oracle_inputs(prog):
    """What the oracle reads of a program besides the source DAG: the leaves
    and the constant pool (not the register allocation)."""
    return [(l.name, l.width) for l in prog.leaves], list(prog.const_values)


def oracle_root_bits(item):
    """Worker (top level, so a spawned process can run it: no GPU state):
    (workload, unit, first, n) -> (the oracle's root bits of the bench unit
    on candidates [first, first + n), ``oracle_inputs`` of the 16-slot
    program it ran on)."""
    from oracle import evalref
    workload, unit, first, n = item
    prog = bench.compile_unit((workload, unit, 16))[1]
    roots = bench.workload_roots(workload, unit)
    want = evalref.run_gen(evalref.serialize(roots, prog), prog, bench.SEED, unit, first, n, 1)
    return np.asarray(want, dtype=bool)[:n], oracle_inputs(prog)
