"""The four-wave register layout (11 slots: the library's second
interpreter) that bench.py runs the C2 corpus on (chosen per batch by
mythril_amd/layout.py): a small default-shaped C2 bench whose
self-check compares the root bits and first satisfying indices of its own
launch with oracle/evalref.c; and both layouts launched from one process.
(The whole bench configuration on both layouts: tests/test_gpu_bench_parity.py.)"""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.gpu
def test_c2_four_wave_layout_self_check():
    env = dict(os.environ)
    for k in ("MYTHGPU_NREG", "MYTHGPU_LDS_SLOTS", "MYTHGPU_LIB", "MYTHGPU_JIT_CACHE"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, "-u", "bench.py", "--workload", "c2", "--dags", "256",
                        "--steps", "1", "--warmup", "0", "--assign-log2", "16", "--full"],
                       cwd=ROOT, env=env, capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-4000:])
    d = json.loads(r.stdout[r.stdout.rindex('{"metric"'):])
    assert d["config"]["register_layout"] == "11 slots, 4 waves/SIMD, 5 LDS regions"
    assert d["config"]["layout_rule"]["nreg"] == 11 and not d["config"]["layout_rule"]["explicit"]
    assert d["runtime"]["library"] == "libmythgpu.so"
    sc = d["selfcheck"]
    assert sc["dags"] > 0 and sc["lanes"] > 0
    assert sc["mismatches"] == 0 and sc["first_sat_mismatches"] == 0


@pytest.mark.gpu
def test_both_layouts_in_one_process():
    """one process, one library, two contexts — the
    16-slot and the 11-slot interpreter — each launched on a batch compiled
    for it (interpreted and compiled code); both give the oracle's root bits
    and first satisfying indices, a program of one layout is refused by the
    other's context, and the layout rule picks 11 for the C2 batch and 16 for
    the C3 batch."""
    import bench
    import gpu_batch as G
    from mythril_amd import jit, layout
    from mythril_amd.engine import EngineError, get_engine
    from mythril_amd.procmap import process_map
    from test_gpu_bench_parity import FIRST, N_LANES, SEED

    units = [("c2", d) for d in range(0, 4096, 256)] + [("c3", d) for d in range(0, 256, 32)]
    oracle = dict(zip(units, process_map(G.oracle_root_bits,
                                         [u + (FIRST, N_LANES) for u in units], 8, "spawn")))
    e16, e11 = get_engine(0, nreg=16), get_engine(0, nreg=11)
    assert (e16.nreg, e11.nreg, e16.lds_slots, e11.lds_slots) == (16, 11, 6, 5)
    for w in ("c2", "c3"):
        ids = [d for ww, d in units if ww == w]
        p16 = [bench.compile_unit((w, d, 16))[1] for d in ids]
        assert layout.choose(p16) == (11 if w == "c2" else 16)
        for nreg, eng in ((16, e16), (11, e11)):
            progs = [(d, bench.compile_unit((w, d, nreg))[1]) for d in ids]
            assert all(G.oracle_inputs(p) == oracle[(w, d)][1] for d, p in progs)
            for image in (None, jit.compile_batch([(p, None, d) for d, p in progs])):
                bits, firsts = G.run_batch(eng, progs, SEED, FIRST, N_LANES, image)
                G.assert_matches_oracle(bits, firsts, [oracle[(w, d)][0] for d in ids], FIRST,
                                        (w, nreg, image is not None), ids)
    p16 = bench.compile_unit(("c2", 0, 16))[1]
    with pytest.raises(EngineError, match="register slots"):
        e11.load(p16)

