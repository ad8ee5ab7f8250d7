"""ctypes binding of libmythgpu (include/mythgpu.h).

The product path has no CPU evaluator: if the shared library or the GPU is
missing, :func:`get_engine` raises :class:`EngineUnavailable` and the caller
(``mythril_amd.model.get_model``) falls back to z3 — never to a host
re-implementation.
"""

from __future__ import annotations

import ctypes as C
import os
import threading
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from .ir import Program


def _default_lib() -> str:
    from .build import LIB
    return LIB


# One library holds the interpreter of every register layout (build.LAYOUTS;
# a context runs one, Engine(nreg=...)).  MYTHGPU_LIB: an A/B build of the
# same ABI.
_LIB_PATH = os.environ.get("MYTHGPU_LIB") or _default_lib()

EXPORTS = ("mg_init", "mg_init_layout", "mg_layouts", "mg_free", "mg_last_error",
           "mg_device_info", "mg_load_program", "mg_free_program", "mg_eval", "mg_eval_gen",
           "mg_search", "mg_batch_create", "mg_batch_free", "mg_batch_eval_gen", "mg_batch_search",
           "mg_batch_search_probes", "mg_keccak256", "mg_version", "mg_config", "mg_translate",
           "mg_asm_digest", "mg_asm_digest_layout", "mg_last_kernel_ms", "mg_jit_attach",
           "mg_jit_detach", "mg_runtime_info", "mg_census", "mg_repair", "mg_repair_mutate_host",
           "mg_walk", "mg_walk_score_host", "mg_walk_tree", "mg_walk_tree_score_host",
           "mg_walk_aim", "mg_walk_aim_mutate_host", "mg_walk_bound",
           "mg_walk_bound_mutate_host", "mg_walk_uf", "mg_walk_uf_resolve_host",
           "mg_walk_uf_mutate_host", "mg_walk_sum", "mg_walk_sum_mutate_host", "mg_walk_batch",
           "mg_walk_batch_plan_host", "mg_walk_batch_shape_ok_host", "mg_census_batch",
           "mg_census_batch_plan_host", "mg_census_batch_blocks_host", "mg_batch_witness",
           "mg_carry_batch", "mg_carry_fill_host", "mg_carry_plan_host", "mg_carry_ladder",
           "mg_carry_fill_rungs_host", "mg_carry_ladder_plan_host", "mg_carry_census",
           "mg_carry_census_plan_host", "mg_carry_starts_host", "mg_carry_ladder_sets",
           "mg_carry_fill_sets_host", "mg_carry_sets_plan_host")


def layouts() -> Dict[int, Tuple[int, int]]:
    """slots -> (waves per SIMD, default LDS spill regions) of every register
    layout the library holds (mg_layouts; build.LAYOUTS)."""
    lib = load_library(check_digest=False)
    buf = (C.c_uint32 * 24)()
    n = lib.mg_layouts(buf, 24)
    return {int(buf[3 * i]): (int(buf[3 * i + 1]), int(buf[3 * i + 2])) for i in range(n)}


def lds_slots_for(nreg: int) -> int:
    """LDS spill regions a context of the ``nreg``-slot layout uses (the
    compiled programs of a batch are rendered for the same): the layout's
    default, or ``MYTHGPU_LDS_SLOTS``."""
    from . import irdefs
    if "MYTHGPU_LDS_SLOTS" in os.environ:
        return irdefs.check_lds_slots(os.environ["MYTHGPU_LDS_SLOTS"])
    from .build import LAYOUT_LDS_SLOTS
    return LAYOUT_LDS_SLOTS[nreg]


class EngineUnavailable(RuntimeError):
    """No usable engine; ``slot`` > 0 when only an extra context of a device
    (model.DEVICES listing it again) could not be created."""

    def __init__(self, msg: str = "", slot: int = 0, device: int = 0):
        super().__init__(msg)
        self.slot = slot
        self.device = device


class EngineError(RuntimeError):
    pass


class LeafGen(C.Structure):
    _fields_ = [("width", C.c_uint32), ("pool_off", C.c_uint32), ("pool_n", C.c_uint32),
                ("pct_uniform", C.c_uint32), ("pct_small", C.c_uint32),
                ("pct_boundary", C.c_uint32)]


class Gen(C.Structure):
    _fields_ = [("seed", C.c_uint64), ("first_index", C.c_uint64)]


_WALK_COUNTS = ("n_roots", "mask_probe0", "n_atoms", "n_code", "n_resid", "n_entries", "n_pieces",
                "n_srows", "n_slots", "n_funcs", "n_cands", "n_ukeys", "n_urows")


_WALK_TABLES = ("starts", "roots", "atoms", "code", "entries", "pieces", "fixed", "lin", "slots",
                "funcs", "cands", "ukeys")


class WalkJob(C.Structure):
    """mg_walk_job (include/mythgpu.h): one job of mg_walk_batch."""
    _fields_ = [(n, C.c_void_p) for n in (
        "prog", "starts", "roots", "atoms", "code", "entries", "pieces", "fixed", "lin", "slots",
        "funcs", "cands", "ukeys", "out_leaves", "out_nfail", "out_cost", "out_rounds", "trace",
        "out_winner")] + [("seed", C.c_uint64)] + [(n, C.c_uint32) for n in _WALK_COUNTS]


class WalkShape(C.Structure):
    """mg_walk_shape: the counts that size a job's share of the batch's
    device buffer."""
    _fields_ = [(n, C.c_uint32) for n in ("n_leaves", "n_probes") + _WALK_COUNTS]


class CensusJob(C.Structure):
    """mg_census_job (include/mythgpu.h): one job of mg_census_batch."""
    _fields_ = [("prog", C.c_void_p), ("n_roots", C.c_uint32), ("mask_probe0", C.c_uint32)]


class CensusShape(C.Structure):
    """mg_census_shape: the counts that size a job's share of the census
    batch's device buffer."""
    _fields_ = [(n, C.c_uint32) for n in ("n_probes", "n_roots", "mask_probe0")]


class CarryJob(C.Structure):
    """mg_carry_job (include/mythgpu.h): one job of mg_carry_batch."""
    _fields_ = [("prog", C.c_void_p), ("pin_rows", C.c_void_p), ("pin_mask", C.c_void_p)]


class CarryLadderJob(C.Structure):
    """mg_carry_ladder_job (include/mythgpu.h): one job of mg_carry_ladder."""
    _fields_ = [("prog", C.c_void_p), ("pin_rows", C.c_void_p), ("pin_masks", C.c_void_p),
                ("n_rungs", C.c_uint32), ("pad", C.c_uint32)]


class CarrySetsJob(C.Structure):
    """mg_carry_sets_job (include/mythgpu.h): one job of mg_carry_ladder_sets."""
    _fields_ = [("prog", C.c_void_p), ("pin_rows", C.c_void_p), ("pin_masks", C.c_void_p),
                ("rung_set", C.c_void_p), ("n_rungs", C.c_uint32), ("n_sets", C.c_uint32)]


class CarryCensusJob(C.Structure):
    """mg_carry_census_job (include/mythgpu.h): one job of mg_carry_census."""
    _fields_ = [("ladder", CarryLadderJob), ("n_roots", C.c_uint32), ("mask_probe0", C.c_uint32)]


# include/mythgpu.h
CARRY_MAX_JOBS = 256
CARRY_MAX_RUNGS = 8
CARRY_MAX_LANES = 1 << 20
CARRY_SHARED = 4
CARRY_JOB_REGIONS = 4
CARRY_MAX_WALKERS = 64
CARRY_CENSUS_SHARED = 1
CARRY_CENSUS_JOB_REGIONS = 2
CARRY_MAX_SETS = 8
CARRY_SETS_SHARED = 1
CARRY_SETS_JOB_REGIONS = 1
CENSUS_BATCH_MAX_JOBS = 256
CENSUS_BATCH_SHARED = 2
CENSUS_BATCH_JOB_REGIONS = 2
WALK_BATCH_MAX_JOBS = 256
WALK_BATCH_DEFAULT_BYTES = 1 << 30
WALK_BATCH_SHARED = 5
WALK_BATCH_JOB_REGIONS = 22


_libs: Dict[str, object] = {}
_lib_lock = threading.Lock()


def load_library(path: str = _LIB_PATH, check_digest: bool = True):
    """Load libmythgpu.so (no GPU needed) and declare every export.  Other
    paths (A/B builds of the same ABI) load side by side."""
    with _lib_lock:
        if path in _libs:
            return _libs[path]
        if not os.path.exists(path):
            raise EngineUnavailable("libmythgpu.so not built (%s); run "
                                    "`python -m mythril_amd.build`" % path)
        try:
            lib = C.CDLL(path)
        except OSError as e:            # e.g. the HIP runtime it links is missing
            raise EngineUnavailable("cannot load %s: %s" % (path, e)) from e
        p, u32, u64, i64 = C.c_void_p, C.c_uint32, C.c_uint64, C.c_int64
        lib.mg_version.restype = C.c_int
        lib.mg_init.argtypes = [C.c_int, C.POINTER(p)]
        lib.mg_init_layout.argtypes = [C.c_int, u32, C.POINTER(p)]
        lib.mg_layouts.argtypes = [p, u32]
        lib.mg_asm_digest_layout.argtypes = [u32]
        lib.mg_asm_digest_layout.restype = C.c_char_p
        lib.mg_free.argtypes = [p]
        lib.mg_free.restype = None
        lib.mg_last_error.argtypes = [p]
        lib.mg_last_error.restype = C.c_char_p
        lib.mg_device_info.argtypes = [p, C.c_char_p, C.c_size_t, C.POINTER(C.c_int)]
        lib.mg_load_program.argtypes = [p, p, u32, p, u32, p, u32, u32, u32, u64, C.POINTER(p)]
        lib.mg_free_program.argtypes = [p]
        lib.mg_free_program.restype = None
        lib.mg_eval.argtypes = [p, p, p, u64, p, p]
        lib.mg_eval_gen.argtypes = [p, p, C.POINTER(Gen), u64, p, p, p]
        lib.mg_search.argtypes = [p, p, C.POINTER(Gen), u64, C.POINTER(i64), p]
        lib.mg_census.argtypes = [p, p, C.POINTER(Gen), u64, u32, u32, u64, p, p, p, p, p,
                                  C.POINTER(u32), C.POINTER(i64)]
        lib.mg_repair.argtypes = [p, p, p, u32, u32, u64, u32, u32, u32, p, C.POINTER(u32),
                                  C.POINTER(u32), p]
        lib.mg_repair_mutate_host.argtypes = [p, u32, p, u32, p, u64, u32, u32, u32, u32, p, p]
        lib.mg_walk.argtypes = [p, p, p, u32, u32, u32, p, u32, u64, u32, u32, u32, p, p, p,
                                C.POINTER(u32), p, C.POINTER(u32)]
        lib.mg_walk_score_host.argtypes = [p, p, p, u32, u32, u64, p, p]
        lib.mg_walk_tree.argtypes = [p, p, p, u32, u32, u32, p, u32, p, p, u32, u32, u64, u32, u32,
                                     u32, p, p, p, C.POINTER(u32), p, C.POINTER(u32)]
        lib.mg_walk_tree_score_host.argtypes = [p, p, p, p, u32, p, u32, p, u32, u32, u64, p, p]
        lib.mg_walk_aim.argtypes = [p, p, p, u32, u32, u32, p, u32, p, p, u32, u32, p, u32, p, u32,
                                    u64, u32, u32, u32, p, p, p, C.POINTER(u32), p, C.POINTER(u32)]
        lib.mg_walk_aim_mutate_host.argtypes = [p, u32, p, u32, p, p, u32, p, u32, p, u32, u64, u32,
                                                u32, u32, u32, p, p]
        lib.mg_walk_bound.argtypes = [p, p, p, u32, u32, u32, p, u32, p, p, u32, u32, p, u32, p,
                                      u32, p, u64, u32, u32, u32, p, p, p, C.POINTER(u32), p,
                                      C.POINTER(u32)]
        lib.mg_walk_bound_mutate_host.argtypes = [p, u32, p, u32, p, p, u32, p, u32, u32, p, u32,
                                                  p, u32, p, u64, u32, u32, u32, u32, p, p]
        lib.mg_walk_uf.argtypes = [p, p, p, u32, u32, u32, p, u32, p, p, u32, u32, p, u32, p, u32,
                                   p, p, u32, p, u32, p, u32, p, u32, u32, u64, u32, u32, u32, p,
                                   p, p, C.POINTER(u32), p, C.POINTER(u32)]
        lib.mg_walk_uf_resolve_host.argtypes = [p, u32, p, p, u32, p, u32, p, u32, p, u32, p, u32,
                                                p]
        lib.mg_walk_uf_mutate_host.argtypes = [p, u32, p, u32, p, p, u32, p, u32, u32, p, u32, p,
                                               u32, p, p, u32, p, u32, p, u32, p, u32, u32, p,
                                               u64, u32, u32, u32, u32, p, p]
        lib.mg_walk_sum.argtypes = [p, p, p, u32, u32, u32, p, u32, p, p, u32, u32, p, u32, p, u32,
                                    p, p, u32, p, u32, p, u32, p, u32, p, u32, u32, u64, u32, u32,
                                    u32, p, p, p, C.POINTER(u32), p, C.POINTER(u32)]
        lib.mg_walk_sum_mutate_host.argtypes = [p, u32, p, u32, p, p, u32, p, u32, u32, p, u32, p,
                                                u32, p, p, p, u32, p, u32, p, u32, p, u32, p, u32,
                                                u32, p, u64, u32, u32, u32, u32, p, p]
        lib.mg_walk_batch.argtypes = [p, C.POINTER(WalkJob), u32, u32, u32, u32, u32, u64]
        lib.mg_walk_batch_plan_host.argtypes = [C.POINTER(WalkShape), u32, u32, u32, u32, p,
                                                C.POINTER(u64)]
        lib.mg_walk_batch_shape_ok_host.argtypes = [C.POINTER(WalkShape)]
        lib.mg_census_batch.argtypes = [p, C.POINTER(CensusJob), u32, C.POINTER(Gen), u64, u64, u32,
                                        p, p, p, p, p, p, p]
        lib.mg_census_batch_plan_host.argtypes = [C.POINTER(CensusShape), u32, u64, u64, p,
                                                  C.POINTER(u64), C.POINTER(u64), C.c_char_p,
                                                  C.c_size_t]
        lib.mg_census_batch_blocks_host.argtypes = [u32, u64]
        lib.mg_batch_witness.argtypes = [p, C.POINTER(p), p, u32, u64, p, u32, p, u32]
        lib.mg_carry_batch.argtypes = [p, C.POINTER(CarryJob), u32, C.POINTER(Gen), u32, p, p, u32,
                                       p]
        lib.mg_carry_fill_host.argtypes = [p, u32, p, u32, u64, p, p, u64, u64, u32, u32, u32, p, p]
        lib.mg_carry_plan_host.argtypes = [p, u32, u32, u32, p, C.POINTER(u64), C.POINTER(u64)]
        lib.mg_carry_ladder.argtypes = [p, C.POINTER(CarryLadderJob), u32, C.POINTER(Gen), u32, p,
                                        p, p, u32, p]
        lib.mg_carry_fill_rungs_host.argtypes = [p, u32, p, u32, u64, p, p, u32, u64, u64, u32, u32,
                                                 u32, u32, p]
        lib.mg_carry_ladder_plan_host.argtypes = [p, p, u32, u32, u32, p, C.POINTER(u64),
                                                  C.POINTER(u64)]
        lib.mg_carry_census.argtypes = [p, C.POINTER(CarryCensusJob), u32, C.POINTER(Gen), u32, u32,
                                        u32, u32, p, p, p, p, p]
        lib.mg_carry_census_plan_host.argtypes = [p, p, p, p, p, u32, u32, u32, u32, p,
                                                  C.POINTER(u64), C.POINTER(u64), C.POINTER(u64)]
        lib.mg_carry_starts_host.argtypes = [p, u32, u32, u32, p, p]
        lib.mg_carry_ladder_sets.argtypes = [p, C.POINTER(CarrySetsJob), u32, C.POINTER(Gen), u32,
                                             p, p, p, u32, p]
        lib.mg_carry_fill_sets_host.argtypes = [p, u32, p, u32, u64, p, p, p, u32, u32, u64, u64,
                                                u32, u32, u32, u32, p]
        lib.mg_carry_sets_plan_host.argtypes = [p, p, p, u32, u32, u32, p, C.POINTER(u64),
                                                C.POINTER(u64)]
        lib.mg_batch_create.argtypes = [p, C.POINTER(p), u32, C.POINTER(p)]
        lib.mg_batch_free.argtypes = [p]
        lib.mg_batch_free.restype = None
        lib.mg_batch_eval_gen.argtypes = [p, p, u64, u64, u64, p, p, p]
        lib.mg_batch_search.argtypes = [p, p, C.POINTER(Gen), u64, p, p, u32]
        lib.mg_batch_search_probes.argtypes = [p, p, C.POINTER(Gen), u64, p, p, u32, p, u32]
        lib.mg_keccak256.argtypes = [p, p, p, p, u32, p]
        lib.mg_config.argtypes = [p, u32]
        lib.mg_asm_digest.restype = C.c_char_p
        lib.mg_last_kernel_ms.argtypes = [p]
        lib.mg_last_kernel_ms.restype = C.c_float
        lib.mg_jit_attach.argtypes = [p, C.POINTER(p), u32, p, C.c_size_t, C.POINTER(p)]
        lib.mg_jit_detach.argtypes = [p]
        lib.mg_jit_detach.restype = None
        lib.mg_runtime_info.argtypes = [C.POINTER(C.c_int), C.c_char_p, C.c_size_t]
        pu32 = C.POINTER(u32)
        lib.mg_translate.argtypes = [p, u32, u32, u32, u32, p, u32, p, u32, pu32, p, u32, pu32]
        for name in EXPORTS:
            getattr(lib, name)
        if check_digest:
            # every layout's interpreter must be the one this generator
            # makes (a stale build is refused; ADVICE r5: and the slot count
            # the compiler allocates must be a layout the library holds)
            from . import asmgen
            from .build import LAYOUTS
            for nreg in sorted(LAYOUTS):
                with asmgen.layout(nreg):
                    want = asmgen.digest()
                got = lib.mg_asm_digest_layout(nreg)
                got = got.decode() if got else None
                if got != want:
                    raise EngineUnavailable(
                        "%s was built from a different assembly interpreter for %d slots "
                        "(digest %s, generator %s); rebuild with `python -m mythril_amd.build`"
                        % (path, nreg, got, want))
            _libs[path] = lib
        return lib


def _ptr(a: Optional[np.ndarray]):
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def default_leafgen(program: Program, pct=(50, 70, 85)) -> List[LeafGen]:
    """C2 value distribution: 50 % uniform, 20 % < 2^64, 15 %
    boundary values, 15 % DAG constants +-1 (pool = the program's constants)."""
    n_c = len(program.const_values)
    widths = getattr(program.leaves, "widths", None) or [l.width for l in program.leaves]
    return [LeafGen(w, 0, n_c, pct[0], pct[1], pct[2]) for w in widths]


class LoadedProgram:
    def __init__(self, engine: "Engine", program: Program, handle):
        self.engine = engine
        self.program = program
        self.handle = handle

    def __del__(self):
        try:
            if self.handle and self.engine._ctx:
                self.engine.lib.mg_free_program(self.handle)
        except Exception:
            pass
        self.handle = None


class Engine:
    """One HIP device context (one per host thread)."""

    def __init__(self, device: int = 0, lib_path: str = _LIB_PATH, nreg: Optional[int] = None):
        """A context on ``device`` running the ``nreg``-slot register layout
        (default: the process's, ``irdefs.NREG``; 16, or 11 for four waves
        per SIMD): programs compiled for that many slots load into it."""
        # an A/B build elsewhere may carry another assembly interpreter
        self.lib = load_library(lib_path, check_digest=lib_path == _LIB_PATH)
        ctx = C.c_void_p()
        from . import irdefs
        self.nreg = irdefs.NREG if nreg is None else int(nreg)
        try:
            self.lds_slots = lds_slots_for(self.nreg)     # (mg_init refuses a bad one too)
        except (KeyError, ValueError) as e:
            raise EngineUnavailable("register layout %d / MYTHGPU_LDS_SLOTS: %s"
                                    % (self.nreg, e)) from e
        rc = self.lib.mg_init_layout(device, self.nreg, C.byref(ctx))
        if rc != 0:
            raise EngineUnavailable("mg_init_layout(%d, %d) failed with %d (no usable GPU?)"
                                    % (device, self.nreg, rc))
        self._ctx = ctx
        name = C.create_string_buffer(256)
        cus = C.c_int()
        self.lib.mg_device_info(ctx, name, 256, C.byref(cus))
        self.device_name = name.value.decode()
        self.n_cus = cus.value

    def close(self):
        if self._ctx:
            self.lib.mg_free(self._ctx)
            self._ctx = None

    def _check(self, rc: int, what: str):
        if rc != 0:
            raise EngineError("%s failed (%d): %s" % (what, rc,
                              self.lib.mg_last_error(self._ctx).decode(errors="replace")))

    def runtime_info(self) -> dict:
        """The HIP runtime the library runs on in this process (version,
        libamdhip64 file)."""
        v = C.c_int()
        path = C.create_string_buffer(1024)
        self.lib.mg_runtime_info(C.byref(v), path, 1024)
        return {"hip_runtime_version": v.value, "libamdhip64": path.value.decode()}

    def last_kernel_ms(self) -> float:
        """Device time of the last synchronous eval / search call."""
        return float(self.lib.mg_last_kernel_ms(self._ctx))

    def load(self, program: Program, leafgen: Optional[Sequence[LeafGen]] = None,
             prog_seed: int = 0) -> LoadedProgram:
        if program.nreg != self.nreg:
            raise EngineError("program compiled for %d register slots, this context runs the "
                              "%d-slot layout" % (program.nreg, self.nreg))
        code = np.ascontiguousarray(program.code, dtype=np.uint32)
        consts = np.ascontiguousarray(program.consts, dtype=np.uint32)
        gens = list(leafgen) if leafgen is not None else default_leafgen(program)
        garr = (LeafGen * max(1, len(gens)))(*gens)
        h = C.c_void_p()
        rc = self.lib.mg_load_program(self._ctx, _ptr(code), code.shape[0], _ptr(consts),
                                      consts.shape[0], C.cast(garr, C.c_void_p), len(gens),
                                      program.n_lds, program.n_probes, prog_seed & (2**64 - 1),
                                      C.byref(h))
        self._check(rc, "mg_load_program")
        return LoadedProgram(self, program, h)

    def eval(self, lp: LoadedProgram, leaves_soa: np.ndarray, want_probes: bool = False):
        """leaves_soa: (n_leaves, 8, n) uint32.  Returns (root bool array,
        probes (n_probes, 8, n) uint32 or None)."""
        prog = lp.program
        leaves_soa = np.ascontiguousarray(leaves_soa, dtype=np.uint32)
        n = leaves_soa.shape[2] if leaves_soa.ndim == 3 else 0
        if leaves_soa.shape[:2] != (len(prog.leaves), 8):
            raise ValueError("leaves_soa must be (n_leaves, 8, n)")
        bits = np.zeros((n + 63) // 64, dtype=np.uint64)
        probes = np.zeros((prog.n_probes, 8, n), dtype=np.uint32) if want_probes else None
        rc = self.lib.mg_eval(self._ctx, lp.handle, _ptr(leaves_soa), n, _ptr(bits), _ptr(probes))
        self._check(rc, "mg_eval")
        return unpack_bits(bits, n), probes

    def eval_gen(self, lp: LoadedProgram, seed: int, first_index: int, n: int,
                 want_probes: bool = False, want_leaves: bool = False):
        prog = lp.program
        bits = np.zeros((n + 63) // 64, dtype=np.uint64)
        probes = np.zeros((prog.n_probes, 8, n), dtype=np.uint32) if want_probes else None
        leaves = np.zeros((len(prog.leaves), 8, n), dtype=np.uint32) if want_leaves else None
        g = Gen(seed & (2**64 - 1), first_index)
        rc = self.lib.mg_eval_gen(self._ctx, lp.handle, C.byref(g), n, _ptr(bits), _ptr(probes),
                                  _ptr(leaves))
        self._check(rc, "mg_eval_gen")
        return unpack_bits(bits, n), probes, leaves

    def search(self, lp: LoadedProgram, seed: int, n_cand: int,
               first_index: int = 0) -> Tuple[int, Optional[np.ndarray]]:
        prog = lp.program
        first = C.c_int64(-1)
        wit = np.zeros((max(1, len(prog.leaves)), 8), dtype=np.uint32)
        g = Gen(seed & (2**64 - 1), first_index)
        rc = self.lib.mg_search(self._ctx, lp.handle, C.byref(g), n_cand, C.byref(first),
                                _ptr(wit))
        self._check(rc, "mg_search")
        if first.value < 0:
            return -1, None
        return first.value, wit[:len(prog.leaves)]

    def census(self, lp: LoadedProgram, seed: int, first_index: int, n_cand: int, n_roots: int,
               mask_probe0: int = 0, chunk: int = 0):
        """Per-constraint verdict census (mg_census) of the candidates
        [first_index, first_index + n_cand) of a program that carries its
        verdict mask as probes ``mask_probe0``.. (``census.mask_probes``; load
        the ``census.census_view`` of a search program): a
        :class:`mythril_amd.census.Census`.  ``first_index`` is a multiple of
        64, ``chunk`` (candidates per launch; 0: 2^16) a multiple of 256."""
        from .census import Census
        n_roots = int(n_roots)
        n = max(1, min(n_roots, 1024)) if n_roots > 0 else 1     # (the library refuses the rest)
        u = [np.zeros(n + 1, dtype=np.uint64) for _ in range(4)]
        sole_index = np.full(n, -1, dtype=np.int64)
        best_nfail, best_index = C.c_uint32(0), C.c_int64(-1)
        g = Gen(seed & (2**64 - 1), first_index)
        rc = self.lib.mg_census(self._ctx, lp.handle, C.byref(g), n_cand, max(0, n_roots),
                                mask_probe0, chunk, _ptr(u[0]), _ptr(u[1]), _ptr(u[2]),
                                _ptr(sole_index), _ptr(u[3]), C.byref(best_nfail),
                                C.byref(best_index))
        self._check(rc, "mg_census")
        return Census(n_roots=n_roots, first_index=first_index, n_cand=n_cand,
                      pass_=u[0][:n].astype(np.int64), first_block=u[1][:n].astype(np.int64),
                      sole_block=u[2][:n].astype(np.int64), sole_index=sole_index,
                      nfail_hist=u[3].astype(np.int64), best_nfail=int(best_nfail.value),
                      best_index=int(best_index.value), kernel_ms=self.last_kernel_ms())

    def census_batch(self, jobs, seed: int, first_index: int, n_cand: int, chunk: int = 0):
        """The censuses of several programs over the candidates [first_index,
        first_index + n_cand) in one launch sequence (mg_census_batch,
        DESIGN.md §3.17).  ``jobs``: a list of ``(lp, n_roots, mask_probe0)``,
        the arguments of :meth:`census` that differ per program.  Returns one
        :class:`mythril_amd.census.Census` per job, equal to ``census`` on it
        alone (``kernel_ms``: the device time of the whole launch sequence the
        job ran in).  More jobs than one batch takes, or jobs whose probe
        regions exceed the library's probe buffer at 256 candidates per chunk,
        run as consecutive sub-batches that fit (:func:`split_census_jobs`);
        jobs are independent, so the results do not depend on the split."""
        from .census import Census
        jobs = [(lp, int(r), int(m)) for lp, r, m in jobs]
        if not jobs:
            return []
        shapes = [CensusShape(lp.program.n_probes, max(0, r) & 0xFFFFFFFF, max(0, m) & 0xFFFFFFFF)
                  for lp, r, m in jobs]
        g = Gen(seed & (2**64 - 1), first_index)
        out = []
        for lo, hi in split_census_jobs(shapes):
            n = hi - lo
            arr = (CensusJob * n)()
            for i, (lp, r, m) in enumerate(jobs[lo:hi]):
                arr[i].prog, arr[i].n_roots, arr[i].mask_probe0 = lp.handle, max(0, r), max(0, m)
            width = max(1, min(max(r for _, r, _ in jobs[lo:hi]), 1024))
            u = [np.zeros((n, width), dtype=np.uint64) for _ in range(3)]
            hist = np.zeros((n, width + 1), dtype=np.uint64)
            sole_index = np.full((n, width), -1, dtype=np.int64)
            best_nfail, best_index = np.zeros(n, dtype=np.uint32), np.full(n, -1, dtype=np.int64)
            rc = self.lib.mg_census_batch(self._ctx, arr, n, C.byref(g), n_cand, chunk, width,
                                          _ptr(u[0]), _ptr(u[1]), _ptr(u[2]), _ptr(sole_index),
                                          _ptr(hist), _ptr(best_nfail), _ptr(best_index))
            self._check(rc, "mg_census_batch")
            ms = self.last_kernel_ms()
            for i, (_, r, _) in enumerate(jobs[lo:hi]):
                out.append(Census(n_roots=r, first_index=first_index, n_cand=n_cand,
                                  pass_=u[0][i, :r].astype(np.int64),
                                  first_block=u[1][i, :r].astype(np.int64),
                                  sole_block=u[2][i, :r].astype(np.int64),
                                  sole_index=sole_index[i, :r].copy(),
                                  nfail_hist=hist[i, :r + 1].astype(np.int64),
                                  best_nfail=int(best_nfail[i]), best_index=int(best_index[i]),
                                  kernel_ms=ms))
        return out

    def carry_batch(self, jobs, seed: int, first_index: int, lanes: int, want_fill: bool = False):
        """Remembered witnesses evaluated on eval-form programs, all jobs in
        one launch sequence (mg_carry_batch).  ``jobs``: a
        list of ``(lp, pin_rows, pin_mask)`` — a program loaded with its leaf
        generators, rows ``(n_leaves, 8)`` uint32 and the words of the pin mask
        (``carry.pins`` builds both).  Lane i of a job evaluates the pin rows
        on the pinned leaves and the generator's candidate ``first_index + i``
        on the free ones.  Returns per job ``(first, leaves)``: the lowest lane
        on which every root holds (-1: none) and that lane's leaf rows
        ``(n_leaves, 8)`` (None when there is none); with ``want_fill`` a third
        element, the job's leaf region ``(n_leaves, 8, lanes)`` as the device
        filled it.  More than ``CARRY_MAX_JOBS`` jobs run as consecutive
        batches; jobs are independent, so the results do not depend on the
        split."""
        jobs = [(lp, np.ascontiguousarray(r, dtype=np.uint32).reshape(-1, 8),
                 np.ascontiguousarray(m, dtype=np.uint32).reshape(-1)) for lp, r, m in jobs]
        for lp, r, m in jobs:
            n = len(lp.program.leaves)
            if r.shape[0] != n or m.shape[0] != (n + 31) // 32:
                raise ValueError("pin rows must be (n_leaves, 8) and the pin mask "
                                 "(n_leaves + 31) // 32 words")
        g = Gen(seed & (2**64 - 1), first_index)
        out = []
        for lo in range(0, len(jobs), CARRY_MAX_JOBS):
            part = jobs[lo:lo + CARRY_MAX_JOBS]
            n = len(part)
            arr = (CarryJob * n)()
            for i, (lp, r, m) in enumerate(part):
                arr[i].prog, arr[i].pin_rows, arr[i].pin_mask = lp.handle, _ptr(r), _ptr(m)
            counts = [len(lp.program.leaves) for lp, _, _ in part]
            max_leaves = max(1, max(counts))
            first = np.full(n, -1, dtype=np.int64)
            wit = np.zeros((n, max_leaves, 8), dtype=np.uint32)
            fill = None
            if want_fill:
                _, _, stride = carry_plan_host(counts, lanes, max_leaves)
                fill = np.zeros((n, max(1, stride)), dtype=np.uint32)
            rc = self.lib.mg_carry_batch(self._ctx, arr, n, C.byref(g), lanes, _ptr(first),
                                         _ptr(wit), max_leaves, _ptr(fill))
            self._check(rc, "mg_carry_batch")
            for i, k in enumerate(counts):
                f = int(first[i])
                res = (f, wit[i, :k].copy() if f >= 0 else None)
                if want_fill:
                    res += (fill[i, :k * 8 * lanes].reshape(k, 8, lanes).copy(),)
                out.append(res)
        return out

    def carry_ladder(self, jobs, seed: int, first_index: int, lanes: int, want_fill: bool = False):
        """:meth:`carry_batch` with a ladder of pin masks per job, all rungs of
        all jobs in one launch sequence (mg_carry_ladder).
        ``jobs``: a list of ``(lp, pin_rows, pin_masks)`` — a program loaded
        with its leaf generators, rows ``(n_leaves, 8)`` uint32 and masks
        ``(n_rungs, (n_leaves + 31) // 32)`` uint32, strictest first, 1 to
        ``CARRY_MAX_RUNGS`` of them (``carry.rungs`` builds both).  With R the
        largest ``n_rungs`` of a batch a job has ``R * lanes`` columns: column
        c lies on rung ``min(c // lanes, n_rungs - 1)`` and evaluates the pin
        rows on the leaves that rung pins and the generator's candidate
        ``first_index + c % lanes`` on the others.  Returns per job ``(first,
        rung, leaves)``: the lowest column on which every root holds, its rung
        (both -1: none) and its leaf rows ``(n_leaves, 8)`` (None when there is
        none); with ``want_fill`` a fourth element, the job's leaf region
        ``(n_leaves, 8, R * lanes)`` as the device filled it.  More than
        ``CARRY_MAX_JOBS`` jobs run as consecutive batches, each with its own
        R; the results do not depend on the split, since a job's lowest true
        column lies below its own ``n_rungs * lanes``."""
        jobs = [(lp, np.ascontiguousarray(r, dtype=np.uint32).reshape(-1, 8),
                 np.ascontiguousarray(m, dtype=np.uint32)) for lp, r, m in jobs]
        for lp, r, m in jobs:
            n = len(lp.program.leaves)
            if r.shape[0] != n or m.ndim != 2 or m.shape[1] != (n + 31) // 32 or \
                    not 1 <= m.shape[0] <= CARRY_MAX_RUNGS:
                raise ValueError("pin rows must be (n_leaves, 8) and the pin masks (n_rungs, "
                                 "(n_leaves + 31) // 32) with 1 to %d rungs" % CARRY_MAX_RUNGS)
        g = Gen(seed & (2**64 - 1), first_index)
        out = []
        for lo in range(0, len(jobs), CARRY_MAX_JOBS):
            part = jobs[lo:lo + CARRY_MAX_JOBS]
            n = len(part)
            arr = (CarryLadderJob * n)()
            for i, (lp, r, m) in enumerate(part):
                arr[i].prog, arr[i].pin_rows, arr[i].pin_masks = lp.handle, _ptr(r), _ptr(m)
                arr[i].n_rungs = m.shape[0]
            counts = [len(lp.program.leaves) for lp, _, _ in part]
            cols = max(m.shape[0] for _, _, m in part) * lanes
            max_leaves = max(1, max(counts))
            first = np.full(n, -1, dtype=np.int64)
            rung = np.full(n, -1, dtype=np.int64)
            wit = np.zeros((n, max_leaves, 8), dtype=np.uint32)
            fill = None
            if want_fill:
                _, _, stride = carry_ladder_plan_host(counts, [m.shape[0] for _, _, m in part],
                                                      lanes, max_leaves)
                fill = np.zeros((n, max(1, stride)), dtype=np.uint32)
            rc = self.lib.mg_carry_ladder(self._ctx, arr, n, C.byref(g), lanes, _ptr(first),
                                          _ptr(rung), _ptr(wit), max_leaves, _ptr(fill))
            self._check(rc, "mg_carry_ladder")
            for i, k in enumerate(counts):
                f = int(first[i])
                res = (f, int(rung[i]), wit[i, :k].copy() if f >= 0 else None)
                if want_fill:
                    res += (fill[i, :k * 8 * cols].reshape(k, 8, cols).copy(),)
                out.append(res)
        return out

    def carry_ladder_sets(self, jobs, seed: int, first_index: int, lanes: int,
                          want_fill: bool = False):
        """:meth:`carry_ladder` with several sets of pin rows per job, every
        rung pinning from a set of its own (mg_carry_ladder_sets, DESIGN.md
        §3.21).  ``jobs``: a list of ``(lp, pin_rows, pin_masks, rung_set)`` —
        rows ``(n_sets, n_leaves, 8)`` uint32 with 1 to ``CARRY_MAX_SETS`` sets,
        masks as :meth:`carry_ladder` takes them and ``rung_set`` ``(n_rungs,)``
        uint32, the row set of every rung, each below ``n_sets``
        (``carry.rungs_sets`` builds the three).  Columns, results,
        ``want_fill`` and the split above ``CARRY_MAX_JOBS`` jobs are
        :meth:`carry_ladder`'s; with one set the results are too."""
        jobs = [(lp, np.ascontiguousarray(r, dtype=np.uint32),
                 np.ascontiguousarray(m, dtype=np.uint32),
                 np.ascontiguousarray(s, dtype=np.uint32)) for lp, r, m, s in jobs]
        for lp, r, m, s in jobs:
            n = len(lp.program.leaves)
            if r.ndim != 3 or r.shape[1:] != (n, 8) or not 1 <= r.shape[0] <= CARRY_MAX_SETS:
                raise ValueError("pin rows must be (n_sets, n_leaves, 8) with 1 to %d sets"
                                 % CARRY_MAX_SETS)
            if m.ndim != 2 or m.shape[1] != (n + 31) // 32 or \
                    not 1 <= m.shape[0] <= CARRY_MAX_RUNGS:
                raise ValueError("the pin masks must be (n_rungs, (n_leaves + 31) // 32) with 1 "
                                 "to %d rungs" % CARRY_MAX_RUNGS)
            if s.shape != (m.shape[0],) or (s >= r.shape[0]).any():
                raise ValueError("rung_set must name one of the job's %d row sets for each of "
                                 "its %d rungs" % (r.shape[0], m.shape[0]))
        g = Gen(seed & (2**64 - 1), first_index)
        out = []
        for lo in range(0, len(jobs), CARRY_MAX_JOBS):
            part = jobs[lo:lo + CARRY_MAX_JOBS]
            n = len(part)
            arr = (CarrySetsJob * n)()
            for i, (lp, r, m, s) in enumerate(part):
                arr[i].prog, arr[i].pin_rows, arr[i].pin_masks = lp.handle, _ptr(r), _ptr(m)
                arr[i].rung_set, arr[i].n_rungs, arr[i].n_sets = _ptr(s), m.shape[0], r.shape[0]
            counts = [len(lp.program.leaves) for lp, _, _, _ in part]
            cols = max(m.shape[0] for _, _, m, _ in part) * lanes
            max_leaves = max(1, max(counts))
            first = np.full(n, -1, dtype=np.int64)
            rung = np.full(n, -1, dtype=np.int64)
            wit = np.zeros((n, max_leaves, 8), dtype=np.uint32)
            fill = None
            if want_fill:
                _, _, stride = carry_sets_plan_host(counts, [m.shape[0] for _, _, m, _ in part],
                                                    [r.shape[0] for _, r, _, _ in part], lanes,
                                                    max_leaves)
                fill = np.zeros((n, max(1, stride)), dtype=np.uint32)
            rc = self.lib.mg_carry_ladder_sets(self._ctx, arr, n, C.byref(g), lanes, _ptr(first),
                                               _ptr(rung), _ptr(wit), max_leaves, _ptr(fill))
            self._check(rc, "mg_carry_ladder_sets")
            for i, k in enumerate(counts):
                f = int(first[i])
                res = (f, int(rung[i]), wit[i, :k].copy() if f >= 0 else None)
                if want_fill:
                    res += (fill[i, :k * 8 * cols].reshape(k, 8, cols).copy(),)
                out.append(res)
        return out

    def carry_census(self, jobs, seed: int, first_index: int, lanes: int, walkers: int,
                     want_fill: bool = False):
        """:meth:`carry_ladder`'s columns, censused per rung, and ``walkers``
        start columns per job, all jobs in one launch sequence
        (mg_carry_census).  ``jobs``: a list of ``(lp,
        pin_rows, pin_masks, n_roots)`` — a ladder job whose program carries
        its verdict mask as its first probes (``census.mask_probes``; load the
        ``census.census_view``).  Returns per job ``(censuses, start_col,
        start_nfail, starts)``: one :class:`mythril_amd.census.Census` per rung
        over the rung's own columns (``first_index = r * lanes``, ``n_cand =
        lanes``: indices are column numbers), and the columns
        (``(walkers,)`` int64), failing roots (uint32) and leaf rows
        (``(walkers, n_leaves, 8)`` uint32) that ``carry.starts_ref`` picks
        from those censuses.  When ``start_nfail[0] == 0``, ``start_col[0]`` is
        :meth:`carry_ladder`'s ``first``, ``start_col[0] // lanes`` its rung
        and ``starts[0]`` its leaves.  With ``want_fill`` a fifth element, the
        job's leaf region.  More than ``CARRY_MAX_JOBS`` jobs run as
        consecutive batches."""
        from .census import unpack_block
        jobs = [(lp, np.ascontiguousarray(r, dtype=np.uint32).reshape(-1, 8),
                 np.ascontiguousarray(m, dtype=np.uint32), int(k)) for lp, r, m, k in jobs]
        for lp, r, m, k in jobs:
            n = len(lp.program.leaves)
            if r.shape[0] != n or m.ndim != 2 or m.shape[1] != (n + 31) // 32 or \
                    not 1 <= m.shape[0] <= CARRY_MAX_RUNGS:
                raise ValueError("pin rows must be (n_leaves, 8) and the pin masks (n_rungs, "
                                 "(n_leaves + 31) // 32) with 1 to %d rungs" % CARRY_MAX_RUNGS)
        g = Gen(seed & (2**64 - 1), first_index)
        w = max(1, min(int(walkers), CARRY_MAX_WALKERS))         # (the library refuses the rest)
        out = []
        for lo in range(0, len(jobs), CARRY_MAX_JOBS):
            part = jobs[lo:lo + CARRY_MAX_JOBS]
            n = len(part)
            arr = (CarryCensusJob * n)()
            for i, (lp, r, m, k) in enumerate(part):
                lad = arr[i].ladder
                lad.prog, lad.pin_rows, lad.pin_masks, lad.n_rungs = \
                    lp.handle, _ptr(r), _ptr(m), m.shape[0]
                arr[i].n_roots, arr[i].mask_probe0 = max(0, k) & 0xFFFFFFFF, 0
            counts = [len(lp.program.leaves) for lp, _, _, _ in part]
            top = max(m.shape[0] for _, _, m, _ in part)
            cols = top * lanes
            max_leaves = max(1, max(counts))
            max_roots = max(1, min(max(k for _, _, _, k in part), 1024))
            blocks = np.zeros((n, top, 5 * max_roots + 2), dtype=np.uint64)
            col = np.full((n, w), -1, dtype=np.int64)
            nfail = np.zeros((n, w), dtype=np.uint32)
            rows = np.zeros((n, w, max_leaves, 8), dtype=np.uint32)
            fill = None
            if want_fill:
                _, _, stride = carry_ladder_plan_host(counts, [m.shape[0] for _, _, m, _ in part],
                                                      lanes, max_leaves)
                fill = np.zeros((n, max(1, stride)), dtype=np.uint32)
            rc = self.lib.mg_carry_census(self._ctx, arr, n, C.byref(g), lanes, walkers, max_roots,
                                          max_leaves, _ptr(blocks), _ptr(col), _ptr(nfail),
                                          _ptr(rows), _ptr(fill))
            self._check(rc, "mg_carry_census")
            ms = self.last_kernel_ms()
            for i, (nl, (_, _, m, k)) in enumerate(zip(counts, part)):
                cs = [unpack_block(blocks[i, r], k, r * lanes, lanes, ms)
                      for r in range(m.shape[0])]
                res = (cs, col[i].copy(), nfail[i].copy(), rows[i, :, :nl].copy())
                if want_fill:
                    res += (fill[i, :nl * 8 * cols].reshape(nl, 8, cols).copy(),)
                out.append(res)
        return out

    def batch_witness(self, pairs, seed: int, want_probes: bool = True):
        """Leaves and probe values of many (program, candidate index) pairs in
        one launch (mg_batch_witness): per pair ``(leaves,
        probes)`` as :meth:`witness` returns them (``probes`` None without
        ``want_probes``).  A program may appear in many pairs; index -1 gives
        zero rows."""
        pairs = [(lp, int(i)) for lp, i in pairs]
        if not pairs:
            return []
        n = len(pairs)
        max_leaves = max(1, max(len(lp.program.leaves) for lp, _ in pairs))
        max_probes = max(1, max(lp.program.n_probes for lp, _ in pairs))
        arr = (C.c_void_p * n)(*[lp.handle for lp, _ in pairs])
        idx = np.array([i for _, i in pairs], dtype=np.int64)
        wit = np.zeros((n, max_leaves, 8), dtype=np.uint32)
        prb = np.zeros((n, max_probes, 8), dtype=np.uint32) if want_probes else None
        rc = self.lib.mg_batch_witness(self._ctx, arr, _ptr(idx), n, seed & (2**64 - 1), _ptr(wit),
                                       max_leaves, _ptr(prb), max_probes)
        self._check(rc, "mg_batch_witness")
        return [(wit[k, :len(lp.program.leaves)].copy(),
                 prb[k, :lp.program.n_probes].copy() if want_probes else None)
                for k, (lp, _) in enumerate(pairs)]

    def repair(self, lp: LoadedProgram, start_leaves: np.ndarray, n_roots: int, seed: int,
               lanes: int = 4096, max_rounds: int = 64, sync_every: int = 8,
               mask_probe0: int = 0):
        """Greedy local search (mg_repair) from ``start_leaves``
        ((n_leaves, 8) u32) on a program that carries its verdict mask as
        probes ``mask_probe0``.. (load the ``census.census_view``): a
        :class:`mythril_amd.repair.RepairResult` — the last base, its failing
        constraints, the rounds run and each round's fewest failing
        constraints."""
        from .repair import RepairResult
        n_leaves = len(lp.program.leaves)
        start = np.ascontiguousarray(start_leaves, dtype=np.uint32)
        if start.shape != (n_leaves, 8):
            raise ValueError("start_leaves must be (n_leaves, 8)")
        out = np.zeros((max(1, n_leaves), 8), dtype=np.uint32)
        trace = np.zeros(max(1, min(int(max_rounds), 1 << 16)), dtype=np.uint32)
        nfail, rounds = C.c_uint32(0), C.c_uint32(0)
        rc = self.lib.mg_repair(self._ctx, lp.handle, _ptr(start) if n_leaves else _ptr(out),
                                max(0, int(n_roots)), mask_probe0, seed & (2**64 - 1), lanes,
                                max_rounds, sync_every, _ptr(out), C.byref(nfail),
                                C.byref(rounds), _ptr(trace))
        self._check(rc, "mg_repair")
        return RepairResult(out[:n_leaves], int(nfail.value), int(rounds.value), trace,
                            self.last_kernel_ms())

    def walk(self, lp: LoadedProgram, starts: np.ndarray, n_roots: int, table: np.ndarray,
             n_resid: int, seed: int, lanes: int = 4096, max_rounds: int = 64,
             sync_every: int = 8, mask_probe0: int = 0):
        """Scored walk (mg_walk) of ``len(starts)`` walkers
        from ``starts`` ((walkers, n_leaves, 8) u32) on a program that carries
        its verdict mask as probes ``mask_probe0``.. and ``n_resid`` residual
        probes right after it (``repair.residuals``, whose ``table`` says
        which root reads which): a :class:`mythril_amd.repair.WalkResult`."""
        n_leaves = len(lp.program.leaves)
        starts = np.ascontiguousarray(starts, dtype=np.uint32)
        if starts.ndim != 3 or starts.shape[1:] != (n_leaves, 8):
            raise ValueError("starts must be (walkers, n_leaves, 8)")
        walkers = starts.shape[0]
        table = np.ascontiguousarray(table, dtype=np.uint32)
        if table.shape != (max(0, int(n_roots)),) and 1 <= int(n_roots) <= 1024:
            raise ValueError("table must have n_roots entries")
        bufs = out, nfail, cost, trace, rounds, winner = _walk_outputs(walkers, n_leaves,
                                                                       max_rounds)
        rc = self.lib.mg_walk(self._ctx, lp.handle, _ptr(starts) if starts.size else _ptr(out),
                              walkers, max(0, int(n_roots)), mask_probe0,
                              _ptr(table) if table.size else _ptr(nfail), max(0, int(n_resid)),
                              seed & (2**64 - 1), lanes, max_rounds, sync_every, _ptr(out),
                              _ptr(nfail), _ptr(cost), C.byref(rounds), _ptr(trace),
                              C.byref(winner))
        self._check(rc, "mg_walk")
        return _walk_result(bufs, n_leaves, self.last_kernel_ms())

    def walk_tree(self, lp: LoadedProgram, starts: np.ndarray, n_roots: int, trees, seed: int,
                  lanes: int = 4096, max_rounds: int = 64, sync_every: int = 8,
                  mask_probe0: int = 0, n_resid: Optional[int] = None):
        """Scored walk with tree distances (mg_walk_tree):
        :meth:`walk` on a program that carries, from probe ``mask_probe0`` on,
        its root mask, the atom mask and the residual probes of ``trees``
        (``repair.distance_trees``; ``n_resid``: how many residual probes the
        program has, by default the trees'): a
        :class:`mythril_amd.repair.WalkResult`."""
        q = _pack_walk(lp, starts, n_roots, trees, mask_probe0=mask_probe0, n_resid=n_resid)
        return self._walk_rung("mg_walk_tree", lp, q, seed, lanes, max_rounds, sync_every)

    def walk_aim(self, lp: LoadedProgram, starts: np.ndarray, n_roots: int, trees, aims, seed: int,
                 lanes: int = 4096, max_rounds: int = 64, sync_every: int = 8,
                 mask_probe0: int = 0, n_resid: Optional[int] = None):
        """Tree-scored walk with aimed moves (mg_walk_aim):
        :meth:`walk_tree` with the aim table ``aims`` (``repair.aim_table``:
        ``entries`` (n, 3) and ``pieces`` (m, 4) u32); with no entry it is
        :meth:`walk_tree` bit for bit."""
        q = _pack_walk(lp, starts, n_roots, trees, aims=aims, mask_probe0=mask_probe0,
                       n_resid=n_resid)
        return self._walk_rung("mg_walk_aim", lp, q, seed, lanes, max_rounds, sync_every)

    def _walk_rung(self, name: str, lp: LoadedProgram, q: dict, seed: int, lanes: int,
                   max_rounds: int, sync_every: int):
        """What the tree-scored walks share: the result buffers and the call of
        the C entry ``name`` on the arrays ``q`` of :func:`_pack_walk`.  The
        entry's argument list has the tables that were packed: the aim or
        bound table, the fixed values, the lin words with the side rows, the
        UF tables with the U rows."""
        s = q["shape"]
        walkers = q["starts"].shape[0]
        bufs = out, nfail, cost, trace, rounds, winner = _walk_outputs(walkers, s.n_leaves,
                                                                       max_rounds)

        def ptr(name, empty=None):
            return _ptr(q[name]) if q[name].size else empty

        args = [self._ctx, lp.handle, ptr("starts", _ptr(out)), walkers, s.n_roots, s.mask_probe0,
                ptr("roots", _ptr(nfail)), s.n_atoms, ptr("atoms"), ptr("code"), s.n_code,
                s.n_resid]
        if q["entries"] is not None:
            args += [ptr("entries"), s.n_entries, ptr("pieces"), s.n_pieces]
        if q["fixed"] is not None:
            args += [ptr("fixed")]
        if q["lin"] is not None:
            args += [ptr("lin"), s.n_srows]
        if q["slots"] is not None:
            args += [*_uf_args([q[k] for k in ("slots", "funcs", "cands", "ukeys")]), s.n_urows]
        args += [seed & (2**64 - 1), lanes, max_rounds, sync_every, _ptr(out), _ptr(nfail),
                 _ptr(cost), C.byref(rounds), _ptr(trace), C.byref(winner)]
        self._check(getattr(self.lib, name)(*args), name)
        return _walk_result(bufs, s.n_leaves, self.last_kernel_ms())

    def walk_bound(self, lp: LoadedProgram, starts: np.ndarray, n_roots: int, trees, bounds,
                   seed: int, lanes: int = 4096, max_rounds: int = 64, sync_every: int = 8,
                   mask_probe0: int = 0, n_resid: Optional[int] = None):
        """Tree-scored walk with moves aimed by equalities and orders
        (mg_walk_bound): :meth:`walk_aim` with the table
        ``bounds`` (``repair.bound_table``: ``entries`` (n, 5), ``pieces``
        (m, 4) and ``fixed`` (n, 8) u32); with XOR entries only it is
        :meth:`walk_aim` bit for bit."""
        q = _pack_walk(lp, starts, n_roots, trees, bounds, mask_probe0=mask_probe0,
                       n_resid=n_resid)
        return self._walk_rung("mg_walk_bound", lp, q, seed, lanes, max_rounds, sync_every)

    def walk_uf(self, lp: LoadedProgram, starts: np.ndarray, n_roots: int, trees, bounds, ufs,
                seed: int, lanes: int = 4096, max_rounds: int = 64, sync_every: int = 8,
                mask_probe0: int = 0, n_resid: Optional[int] = None):
        """Tree-scored walk with aims that write the table entry a UF
        application reads (mg_walk_uf): :meth:`walk_bound`
        whose pieces may name a slot of ``ufs`` (``repair.uf_table``); the
        program writes ``ufs.n_urows`` U rows after the residual probes
        (``repair.uf_view``).  With no slot piece it is :meth:`walk_bound` bit
        for bit."""
        q = _pack_walk(lp, starts, n_roots, trees, bounds, ufs, mask_probe0=mask_probe0,
                       n_resid=n_resid)
        return self._walk_rung("mg_walk_uf", lp, q, seed, lanes, max_rounds, sync_every)

    def walk_sum(self, lp: LoadedProgram, starts: np.ndarray, n_roots: int, trees, bounds, ufs,
                 sums, seed: int, lanes: int = 4096, max_rounds: int = 64, sync_every: int = 8,
                 mask_probe0: int = 0, n_resid: Optional[int] = None):
        """Tree-scored walk with aims through sums, differences, masks and
        shifts (mg_walk_sum): :meth:`walk_uf` whose entries
        may be linear (``sums``: ``repair.Sums``, its ``lin`` words parallel to
        ``bounds.entries``); the program writes ``sums.n_srows`` side rows
        after the residual probes and before the U rows.  With no linear entry
        it is :meth:`walk_uf` bit for bit."""
        q = _pack_walk(lp, starts, n_roots, trees, bounds, ufs, sums, mask_probe0=mask_probe0,
                       n_resid=n_resid)
        return self._walk_rung("mg_walk_sum", lp, q, seed, lanes, max_rounds, sync_every)

    def walk_batch(self, jobs, lanes: int = 4096, max_rounds: int = 64, sync_every: int = 8,
                   max_bytes: Optional[int] = None):
        """The walks of several groups in one launch sequence (mg_walk_batch,
        DESIGN.md §3.16).  ``jobs``: a list of ``(lp, starts, n_roots, trees,
        bounds, ufs, sums, seed[, mask_probe0, n_resid])``, the arguments of
        :meth:`walk_sum` for one program each; every job has the same number
        of walkers.  Returns one :class:`mythril_amd.repair.WalkResult` per
        job, equal to ``walk_sum`` on it alone (``kernel_ms``: the device time
        of the whole launch sequence the job ran in).  When the batch's device
        buffer would exceed ``max_bytes`` (default: the library's, 1 GiB) or
        there are more jobs than one batch takes, consecutive sub-batches that
        fit are run; jobs are independent, so the results do not depend on the
        split.  A single job that does not fit raises :class:`EngineError`."""
        jobs = [tuple(j) for j in jobs]
        if not jobs:
            return []
        packed = [_pack_walk_job(j) for j in jobs]
        walkers = packed[0]["starts"].shape[0]
        if any(q["starts"].shape[0] != walkers for q in packed):
            raise ValueError("every job of a batch has the same number of walkers")
        cap = WALK_BATCH_DEFAULT_BYTES if not max_bytes else int(max_bytes)
        shapes = [q["shape"] for q in packed]
        plannable = 1 <= walkers <= 64 and 1 <= lanes <= 1 << 20 and 1 <= max_rounds <= 1 << 16
        if plannable:
            parts = split_walk_jobs(shapes, walkers, lanes, max_rounds, cap)
        else:                                   # the library says what is wrong
            parts = [(0, min(len(jobs), WALK_BATCH_MAX_JOBS))]
        results = []
        for lo, hi in parts:
            arr = (WalkJob * (hi - lo))()
            outs = []
            for j, q in zip(arr, packed[lo:hi]):
                n_leaves = q["shape"].n_leaves
                bufs = out, nfail, cost, trace, rounds, winner = _walk_outputs(walkers, n_leaves,
                                                                               max_rounds)
                outs.append((bufs, n_leaves))
                j.prog = q["lp"].handle
                for name in _WALK_TABLES:
                    a = q[name]
                    setattr(j, name, a.ctypes.data if a.size else None)
                if not q["starts"].size:
                    j.starts = out.ctypes.data
                if not q["roots"].size:
                    j.roots = nfail.ctypes.data
                j.out_leaves, j.out_nfail, j.out_cost = (out.ctypes.data, nfail.ctypes.data,
                                                         cost.ctypes.data)
                j.out_rounds, j.out_winner = C.addressof(rounds), C.addressof(winner)
                j.trace = trace.ctypes.data
                j.seed = q["seed"] & (2**64 - 1)
                for name in _WALK_COUNTS:
                    setattr(j, name, getattr(q["shape"], name))
            rc = self.lib.mg_walk_batch(self._ctx, arr, hi - lo, walkers, lanes, max_rounds,
                                        sync_every, cap)
            self._check(rc, "mg_walk_batch")
            ms = self.last_kernel_ms()
            results += [_walk_result(bufs, n_leaves, ms) for bufs, n_leaves in outs]
        return results

    def witness(self, lp: LoadedProgram, seed: int, index: int):
        """Leaves and probe values of candidate ``index`` (one lane): what a
        solve-mode program's model needs besides the generated leaves."""
        _, probes, leaves = self.eval_gen(lp, seed, index, 1, want_probes=True, want_leaves=True)
        return leaves[:, :, 0], (probes[:, :, 0] if probes is not None else None)

    def keccak256(self, msgs: Sequence[bytes]) -> List[bytes]:
        n = len(msgs)
        if n == 0:
            return []
        lens = np.array([len(m) for m in msgs], dtype=np.uint32)
        offs = np.zeros(n, dtype=np.uint64)
        offs[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
        data = np.frombuffer(b"".join(msgs) or b"\0", dtype=np.uint8).copy()
        out = np.zeros((n, 32), dtype=np.uint8)
        rc = self.lib.mg_keccak256(self._ctx, _ptr(data), _ptr(offs), _ptr(lens), n, _ptr(out))
        self._check(rc, "mg_keccak256")
        return [bytes(out[i]) for i in range(n)]

    # corpus batches (device pointers; used by bench.py)
    def batch_create(self, loaded: Sequence[LoadedProgram]):
        arr = (C.c_void_p * len(loaded))(*[lp.handle for lp in loaded])
        h = C.c_void_p()
        rc = self.lib.mg_batch_create(self._ctx, arr, len(loaded), C.byref(h))
        self._check(rc, "mg_batch_create")
        return h

    def batch_free(self, h):
        self.lib.mg_batch_free(h)

    def jit_attach(self, loaded: Sequence[LoadedProgram], image: bytes):
        """Point the programs at their compiled code (``jit.compile_batch``
        of the same programs, leaf generators and seeds, in order); returns
        the handle for :meth:`jit_detach`.  Attach before ``batch_create``."""
        arr = (C.c_void_p * len(loaded))(*[lp.handle for lp in loaded])
        buf = C.create_string_buffer(image, len(image))
        h = C.c_void_p()
        rc = self.lib.mg_jit_attach(self._ctx, arr, len(loaded), C.cast(buf, C.c_void_p),
                                    len(image), C.byref(h))
        self._check(rc, "mg_jit_attach")
        return h

    def jit_detach(self, h):
        self.lib.mg_jit_detach(h)

    def batch_eval_gen(self, h, seed: int, first_index: int, n_assign: int,
                       d_root_bits: int = 0, d_first_sat: int = 0, stream: int = 0):
        rc = self.lib.mg_batch_eval_gen(self._ctx, h, seed & (2**64 - 1), first_index, n_assign,
                                        C.c_void_p(d_root_bits or None),
                                        C.c_void_p(d_first_sat or None), C.c_void_p(stream or None))
        self._check(rc, "mg_batch_eval_gen")


    def batch_search(self, loaded: Sequence[LoadedProgram], seed: int, n_cand: int,
                     first_index: int = 0, want_probes: bool = False) -> List[tuple]:
        """Witness search over many programs in shared launches
        (mg_batch_search, witnesses regenerated in one launch); per program
        (index, leaves) or (-1, None) — with ``want_probes`` (index, leaves,
        probes) or (-1, None, None), the probe values coming from the same
        regeneration launch (mg_batch_search_probes)."""
        if not loaded:
            return []
        h = self.batch_create(loaded)
        max_leaves = max(1, max(len(lp.program.leaves) for lp in loaded))
        max_probes = max(1, max(lp.program.n_probes for lp in loaded))
        try:
            first = np.full(len(loaded), -1, dtype=np.int64)
            wit = np.zeros((len(loaded), max_leaves, 8), dtype=np.uint32)
            g = Gen(seed & (2**64 - 1), first_index)
            if want_probes:
                prb = np.zeros((len(loaded), max_probes, 8), dtype=np.uint32)
                rc = self.lib.mg_batch_search_probes(self._ctx, h, C.byref(g), n_cand, _ptr(first),
                                                     _ptr(wit), max_leaves, _ptr(prb), max_probes)
                self._check(rc, "mg_batch_search_probes")
            else:
                rc = self.lib.mg_batch_search(self._ctx, h, C.byref(g), n_cand, _ptr(first),
                                              _ptr(wit), max_leaves)
                self._check(rc, "mg_batch_search")
        finally:
            self.batch_free(h)
        out = []
        for k, (lp, f) in enumerate(zip(loaded, first.tolist())):
            if not want_probes:
                out.append((-1, None) if f < 0 else (f, wit[k, :len(lp.program.leaves)].copy()))
            else:
                out.append((-1, None, None) if f < 0 else
                           (f, wit[k, :len(lp.program.leaves)].copy(),
                            prb[k, :lp.program.n_probes].copy()))
        return out


def translate_records(program: Program, lds_slots: Optional[int] = None):
    """Host-only (no GPU): the records ``mg_load_program`` would upload for
    ``program`` with handler IDS in word 0 (the translator run with an
    identity offset table; the last record is the zeroed prefetch pad), and
    the number of mask entries the translator appended to the constant
    table.  ``lds_slots`` is the context's LDS spill tier (``lds_slots_for``
    the program's layout).  The translator is the one of the program's
    register layout (``Program.nreg``)."""
    from . import asmgen
    if lds_slots is None:
        lds_slots = lds_slots_for(program.nreg)
    lib = load_library()
    code = np.ascontiguousarray(program.code, dtype=np.uint32)
    n_ins = code.shape[0]
    ident = np.arange(asmgen.NUM_HANDLERS, dtype=np.uint32)
    max_rec = (2 * n_ins + 3) * 8
    max_mask = (2 * n_ins + 4) * 16
    rec = np.zeros(max_rec, dtype=np.uint32)
    masks = np.zeros(max_mask, dtype=np.uint32)
    nrw, nmw = C.c_uint32(), C.c_uint32()
    rc = lib.mg_translate(_ptr(code), n_ins, program.consts.shape[0],
                          min(program.n_lds, lds_slots), program.nreg, _ptr(ident),
                          asmgen.NUM_HANDLERS,
                          C.cast(rec.ctypes.data, C.POINTER(C.c_uint32)), max_rec, C.byref(nrw),
                          _ptr(masks), max_mask, C.byref(nmw))
    if rc != 0:
        raise EngineError("mg_translate failed (%d)" % rc)
    return rec[:nrw.value], nmw.value // 8


def record_handlers(program: Program, lds_slots: Optional[int] = None) -> List[int]:
    """The assembly-interpreter handler id of every record, in order."""
    rec, _ = translate_records(program, lds_slots)
    return [int(h) for h in rec[::8][:-1]]       # the last record is a zeroed pad


def handler_variants(program: Program, lds_slots: Optional[int] = None):
    """The set of (family, canonical variant) the program executes (every
    record runs on every lane: programs are straight-line)."""
    from . import asmgen
    out = set()
    hs = record_handlers(program, lds_slots)
    with asmgen.layout(program.nreg):
        for h in hs:
            c = asmgen.canonical(h)
            aop, var = c // (2 * asmgen.NVAR), (c // 2) % asmgen.NVAR
            out.add((asmgen.AOPS[aop], var))
    return out


def repair_mutate_host(leafgen: Sequence[LeafGen], consts: np.ndarray, base: np.ndarray, seed: int,
                       r: int, lanes: int, lane0: int = 0, n_lanes: Optional[int] = None):
    """Host-only (no GPU): ``(neighbours (n_leaves, 8, n_lanes) u32, moves
    (n_lanes, 4) u32)`` of lanes ``lane0``.. of round ``r`` from the library's
    own move function (mg_repair_mutate_host; ``repair.mutate_ref`` is its
    specification)."""
    lib = load_library()
    gens = list(leafgen)
    garr = (LeafGen * max(1, len(gens)))(*gens)
    consts = np.ascontiguousarray(consts, dtype=np.uint32).reshape(-1, 8)
    base = np.ascontiguousarray(base, dtype=np.uint32)
    n_lanes = lanes - lane0 if n_lanes is None else n_lanes
    out = np.zeros((max(1, len(gens)), 8, max(1, n_lanes)), dtype=np.uint32)
    moves = np.zeros((max(1, n_lanes), 4), dtype=np.uint32)
    rc = lib.mg_repair_mutate_host(C.cast(garr, C.c_void_p), len(gens), _ptr(consts),
                                   consts.shape[0], _ptr(base), seed & (2**64 - 1), r, lanes,
                                   lane0, n_lanes, _ptr(out), _ptr(moves))
    if rc != 0:
        raise EngineError("mg_repair_mutate_host failed (%d)" % rc)
    return out[:len(gens), :, :n_lanes], moves[:n_lanes]


def walk_aim_mutate_host(leafgen: Sequence[LeafGen], consts: np.ndarray, base: np.ndarray,
                         rvals: Optional[np.ndarray], aims, seed: int, r: int, lanes: int,
                         lane0: int = 0, n_lanes: Optional[int] = None,
                         n_resid: Optional[int] = None):
    """Host-only (no GPU): ``(neighbours (n_leaves, 8, n_lanes) u32, moves
    (n_lanes, 5) u32)`` of lanes ``lane0``.. of round ``r`` from the library's
    own lane function of mg_walk_aim (mg_walk_aim_mutate_host;
    ``repair.aim_mutate_ref`` is its specification).  ``rvals``: the base's
    residual values (n_resid, 8) u32, None in round 0; ``moves``: the four
    words of :func:`repair_mutate_host`, then the aimed entry or 0xFFFFFFFF."""
    lib = load_library()
    gens = list(leafgen)
    garr = (LeafGen * max(1, len(gens)))(*gens)
    consts = np.ascontiguousarray(consts, dtype=np.uint32).reshape(-1, 8)
    base = np.ascontiguousarray(base, dtype=np.uint32)
    entries = np.ascontiguousarray(aims.entries, dtype=np.uint32).reshape(-1, 3)
    pieces = np.ascontiguousarray(aims.pieces, dtype=np.uint32).reshape(-1, 4)
    if rvals is not None:
        rvals = np.ascontiguousarray(rvals, dtype=np.uint32).reshape(-1, 8)
    if n_resid is None:
        n_resid = rvals.shape[0] if rvals is not None else \
            (int(entries[:, 0].max()) + 1 if entries.size else 0)
    if rvals is not None and rvals.shape[0] < n_resid:
        raise EngineError("mg_walk_aim_mutate_host: rvals shorter than n_resid")
    n_lanes = lanes - lane0 if n_lanes is None else n_lanes
    out = np.zeros((max(1, len(gens)), 8, max(1, n_lanes)), dtype=np.uint32)
    moves = np.zeros((max(1, n_lanes), 5), dtype=np.uint32)
    rc = lib.mg_walk_aim_mutate_host(C.cast(garr, C.c_void_p), len(gens), _ptr(consts),
                                     consts.shape[0], _ptr(base),
                                     _ptr(rvals) if rvals is not None and rvals.size else None,
                                     n_resid, _ptr(entries) if entries.size else None,
                                     entries.shape[0], _ptr(pieces) if pieces.size else None,
                                     pieces.shape[0], seed & (2**64 - 1), r, lanes, lane0, n_lanes,
                                     _ptr(out), _ptr(moves))
    if rc != 0:
        raise EngineError("mg_walk_aim_mutate_host failed (%d)" % rc)
    return out[:len(gens), :, :n_lanes], moves[:n_lanes]


def _walk_mutate_host(name: str, leafgen, consts, base, state, bounds, ufs, sums, seed, r, lanes,
                      lane0, n_lanes, n_resid):
    """What :func:`walk_bound_mutate_host`, :func:`walk_uf_mutate_host` and
    :func:`walk_sum_mutate_host` share: ``state`` and the tables as arrays and
    the call of the C entry ``name``, whose argument list has the lin words and
    side rows when ``sums`` is given and the UF tables, U rows and slot
    destinations when ``ufs`` is."""
    from .repair import bound_mask_words
    lib = load_library()
    gens = list(leafgen)
    garr = (LeafGen * max(1, len(gens)))(*gens)
    consts = np.ascontiguousarray(consts, dtype=np.uint32).reshape(-1, 8)
    base = np.ascontiguousarray(base, dtype=np.uint32)
    entries = np.ascontiguousarray(bounds.entries, dtype=np.uint32).reshape(-1, 5)
    pieces = np.ascontiguousarray(bounds.pieces, dtype=np.uint32).reshape(-1, 4)
    fixed = np.ascontiguousarray(bounds.fixed, dtype=np.uint32).reshape(-1, 8)
    rvals = mvals = svals = None
    n_roots, n_atoms = bounds.n_roots, bounds.n_atoms
    if sums is not None:
        lin = np.ascontiguousarray(sums.lin, dtype=np.uint32).reshape(-1)
    if ufs is not None:
        tabs = _uf_arrays(ufs)
        dest = np.full(max(1, tabs[0].shape[0]), 0xFFFFFFFF, dtype=np.uint32)
    if state is not None:
        rvals = np.ascontiguousarray(state[0], dtype=np.uint32).reshape(-1, 8)
        n_roots, n_atoms = len(state[1]), len(state[2])
        mvals = np.concatenate([bound_mask_words(state[1]), bound_mask_words(state[2]),
                                np.zeros(1, dtype=np.uint32)])
        if ufs is not None:
            dest[:tabs[0].shape[0]] = np.asarray(state[3], dtype=np.uint32)
        if sums is not None:
            svals = np.ascontiguousarray(state[4], dtype=np.uint32).reshape(-1, 8)
            if svals.shape[0] < sums.n_srows:
                raise EngineError("%s: srows shorter than n_srows" % name)
    if n_resid is None:
        n_resid = rvals.shape[0] if rvals is not None else \
            (int(entries[:, 0].max()) + 1 if entries.size else 0)
    if rvals is not None and rvals.shape[0] < n_resid:
        raise EngineError("%s: rvals shorter than n_resid" % name)
    n_lanes = lanes - lane0 if n_lanes is None else n_lanes
    out = np.zeros((max(1, len(gens)), 8, max(1, n_lanes)), dtype=np.uint32)
    moves = np.zeros((max(1, n_lanes), 5), dtype=np.uint32)
    args = [C.cast(garr, C.c_void_p), len(gens), _ptr(consts), consts.shape[0], _ptr(base),
            _ptr(rvals) if rvals is not None and rvals.size else None, n_resid,
            _ptr(mvals) if mvals is not None else None, n_roots, n_atoms,
            _ptr(entries) if entries.size else None, entries.shape[0],
            _ptr(pieces) if pieces.size else None, pieces.shape[0],
            _ptr(fixed) if fixed.size else None]
    if sums is not None:
        args += [_ptr(lin) if lin.size else None,
                 _ptr(svals) if svals is not None and svals.size else None, int(sums.n_srows)]
    if ufs is not None:
        args += [*_uf_args(tabs), int(ufs.n_urows), _ptr(dest)]
    args += [seed & (2**64 - 1), r, lanes, lane0, n_lanes, _ptr(out), _ptr(moves)]
    rc = getattr(lib, name)(*args)
    if rc != 0:
        raise EngineError("%s failed (%d)" % (name, rc))
    return out[:len(gens), :, :n_lanes], moves[:n_lanes]


def walk_bound_mutate_host(leafgen: Sequence[LeafGen], consts: np.ndarray, base: np.ndarray,
                           state, bounds, seed: int, r: int, lanes: int, lane0: int = 0,
                           n_lanes: Optional[int] = None, n_resid: Optional[int] = None):
    """Host-only (no GPU): :func:`walk_aim_mutate_host` for the lane function
    of mg_walk_bound (mg_walk_bound_mutate_host; ``repair.bound_mutate_ref`` is
    its specification).  ``state``: what the walker knows of its base, ``(rvals
    (n_resid, 8) u32, root bits (n_roots,) bool, atom bits (n_atoms,) bool)``,
    None in round 0."""
    return _walk_mutate_host("mg_walk_bound_mutate_host", leafgen, consts, base, state, bounds,
                             None, None, seed, r, lanes, lane0, n_lanes, n_resid)


def _pack_walk(lp, starts, n_roots, trees, bounds=None, ufs=None, sums=None, aims=None,
               mask_probe0=0, n_resid=None):
    """One tree-scored walk as the library takes it: the contiguous u32 array
    of every table in ``_WALK_TABLES`` (None for a table of a rung that was not
    given) and, as ``shape``, its :class:`WalkShape`.  ``aims`` (3-word
    entries) or ``bounds`` (5-word entries and fixed values) is the aim table.
    Only the arrays' shapes are checked here; the library refuses the rest."""
    def u32(a):
        return np.ascontiguousarray(a, dtype=np.uint32)

    n_leaves = len(lp.program.leaves)
    q = dict.fromkeys(_WALK_TABLES)
    q["starts"] = u32(starts)
    if q["starts"].ndim != 3 or q["starts"].shape[1:] != (n_leaves, 8):
        raise ValueError("starts must be (walkers, n_leaves, 8)")
    q["roots"], q["atoms"], q["code"] = u32(trees.roots), u32(trees.atoms), u32(trees.code)
    if q["roots"].shape != (max(0, int(n_roots)),) and 1 <= int(n_roots) <= 1024:
        raise ValueError("trees.roots must have n_roots entries")
    n = n_pieces = 0
    if aims is not None:
        q["entries"], q["pieces"] = u32(aims.entries), u32(aims.pieces)
        if q["entries"].shape[1:] != (3,) or q["pieces"].shape[1:] != (4,):
            raise ValueError("aims.entries must be (n, 3), aims.pieces (m, 4)")
    if bounds is not None:
        q["entries"], q["pieces"], q["fixed"] = (u32(bounds.entries), u32(bounds.pieces),
                                                 u32(bounds.fixed))
        n = q["entries"].shape[0]
        if sums is not None:
            q["lin"] = u32(sums.lin)
        if q["entries"].shape[1:] != (5,) or q["pieces"].shape[1:] != (4,) or \
                q["fixed"].shape != (n, 8) or (sums is not None and q["lin"].shape != (n,)):
            raise ValueError("bounds.entries must be (n, 5), bounds.pieces (m, 4), "
                             "bounds.fixed (n, 8)" + ("" if sums is None else ", sums.lin (n,)"))
    if q["entries"] is not None:
        n, n_pieces = q["entries"].shape[0], q["pieces"].shape[0]
    if ufs is not None:
        q["slots"], q["funcs"], q["cands"], q["ukeys"] = _uf_arrays(ufs)
    n_resid = len(trees.probes) if n_resid is None else n_resid
    q["shape"] = WalkShape(
        n_leaves=n_leaves, n_probes=lp.program.n_probes, n_roots=max(0, int(n_roots)),
        mask_probe0=mask_probe0, n_atoms=q["atoms"].size, n_code=q["code"].size,
        n_resid=max(0, int(n_resid)), n_entries=n, n_pieces=n_pieces,
        n_srows=0 if sums is None else max(0, int(sums.n_srows)),
        n_urows=0 if ufs is None else max(0, int(ufs.n_urows)),
        **{"n_" + k: 0 if q[k] is None else q[k].shape[0]
           for k in ("slots", "funcs", "cands", "ukeys")})
    return q


def _pack_walk_job(job):
    """One job tuple of :meth:`Engine.walk_batch` through :func:`_pack_walk`,
    with its ``lp`` and ``seed``."""
    q = _pack_walk(*job[:7], **dict(zip(("mask_probe0", "n_resid"), job[8:10])))
    q["lp"], q["seed"] = job[0], int(job[7])
    return q


def _walk_outputs(walkers: int, n_leaves: int, max_rounds: int):
    """The buffers one walk writes, ``(out, nfail, cost, trace, rounds,
    winner)``, never empty and never larger than the library's limits: a count
    out of range is for the library to refuse."""
    w1, r1 = max(1, min(walkers, 64)), max(1, min(int(max_rounds), 1 << 16))
    return (np.zeros((w1, max(1, n_leaves), 8), dtype=np.uint32), np.zeros(w1, dtype=np.uint32),
            np.zeros(w1, dtype=np.uint32), np.zeros((w1, r1, 2), dtype=np.uint32),
            C.c_uint32(0), C.c_uint32(0))


def _walk_result(bufs, n_leaves: int, kernel_ms: float):
    """The :class:`mythril_amd.repair.WalkResult` of the buffers of
    :func:`_walk_outputs` after the walk."""
    from .repair import WalkResult
    out, nfail, cost, trace, rounds, winner = bufs
    return WalkResult(out[:, :n_leaves], nfail.astype(np.int64), cost.astype(np.int64),
                      int(rounds.value), trace, int(winner.value), kernel_ms)


def walk_batch_plan_host(shapes: Sequence[WalkShape], walkers: int, lanes: int, max_rounds: int):
    """Host-only (no GPU): ``(offsets, bytes)`` of the device buffer
    mg_walk_batch uses for jobs of these shapes (mg_walk_batch_plan_host:
    ``offsets`` u64, WALK_BATCH_SHARED shared regions and then
    WALK_BATCH_JOB_REGIONS per job), or ``None`` when the library refuses the
    arguments or the size exceeds 64 bits."""
    lib = load_library(check_digest=False)
    n = len(shapes)
    arr = (WalkShape * max(1, n))(*shapes)
    offs = np.zeros(WALK_BATCH_SHARED + max(1, n) * WALK_BATCH_JOB_REGIONS, dtype=np.uint64)
    total = C.c_uint64(0)
    rc = lib.mg_walk_batch_plan_host(arr, n, walkers, lanes, max_rounds, _ptr(offs),
                                     C.byref(total))
    if rc != 0:
        return None
    return offs[:WALK_BATCH_SHARED + n * WALK_BATCH_JOB_REGIONS], int(total.value)


def split_walk_jobs(shapes: Sequence[WalkShape], walkers: int, lanes: int, max_rounds: int,
                    max_bytes: int, max_jobs: int = WALK_BATCH_MAX_JOBS):
    """Consecutive ``(lo, hi)`` ranges that cover ``shapes`` once, in order,
    each the longest run from its start whose plan (:func:`walk_batch_plan_host`)
    stays within ``max_bytes`` and ``max_jobs``.  A plan only grows with
    another job (the strides are maxima), so the greedy run is found by
    extending it.  :class:`EngineError` for a job that does not fit alone."""
    parts, lo, n = [], 0, len(shapes)
    while lo < n:
        hi = lo
        while hi < n and hi - lo < max_jobs:
            plan = walk_batch_plan_host(shapes[lo:hi + 1], walkers, lanes, max_rounds)
            if plan is None or plan[1] > max_bytes:
                break
            hi += 1
        if hi == lo:
            plan = walk_batch_plan_host(shapes[lo:lo + 1], walkers, lanes, max_rounds)
            raise EngineError("walk_batch: job %d alone needs %s bytes, max_bytes is %d"
                              % (lo, "more than 2^64" if plan is None else plan[1], max_bytes))
        parts.append((lo, hi))
        lo = hi
    return parts


def census_batch_plan_host(shapes: Sequence[CensusShape], n_cand: int, chunk: int = 0):
    """Host-only (no GPU): ``(offsets, bytes, chunk)`` of the device buffer
    mg_census_batch uses for jobs of these shapes (mg_census_batch_plan_host:
    ``offsets`` u64, CENSUS_BATCH_SHARED shared regions and then
    CENSUS_BATCH_JOB_REGIONS per job; ``chunk``: the candidates per launch).
    :class:`EngineError` with the library's words when it refuses."""
    lib = load_library(check_digest=False)
    n = len(shapes)
    arr = (CensusShape * max(1, n))(*shapes)
    offs = np.zeros(CENSUS_BATCH_SHARED + max(1, n) * CENSUS_BATCH_JOB_REGIONS, dtype=np.uint64)
    total, got = C.c_uint64(0), C.c_uint64(0)
    why = C.create_string_buffer(512)
    rc = lib.mg_census_batch_plan_host(arr, n, n_cand, chunk, _ptr(offs), C.byref(total),
                                       C.byref(got), why, 512)
    if rc != 0:
        raise EngineError("census_batch: " + why.value.decode(errors="replace"))
    return (offs[:CENSUS_BATCH_SHARED + n * CENSUS_BATCH_JOB_REGIONS], int(total.value),
            int(got.value))


def carry_plan_host(n_leaves: Sequence[int], lanes: int, max_leaves: int):
    """Host-only: ``(offsets, bytes, leaf_stride_words)`` of the device buffer
    mg_carry_batch uses for jobs of these leaf counts (mg_carry_plan_host:
    ``CARRY_SHARED`` shared offsets, then ``CARRY_JOB_REGIONS`` per job — mask,
    rows, generators, leaf region).  :class:`EngineError` where the library
    refuses: counts out of range or sizes beyond 64 bits."""
    lib = load_library(check_digest=False)
    counts = np.ascontiguousarray(n_leaves, dtype=np.uint32)
    n = counts.shape[0]
    offs = np.zeros(CARRY_SHARED + max(1, n) * CARRY_JOB_REGIONS, dtype=np.uint64)
    total, stride = C.c_uint64(0), C.c_uint64(0)
    rc = lib.mg_carry_plan_host(_ptr(counts), n, lanes, max_leaves, _ptr(offs), C.byref(total),
                                C.byref(stride))
    if rc != 0:
        raise EngineError("carry_batch: %d jobs at %d lanes: counts out of range or a buffer "
                          "beyond 64 bits" % (n, lanes))
    return offs[:CARRY_SHARED + n * CARRY_JOB_REGIONS], int(total.value), int(stride.value)


def carry_fill_host(leafgen: Sequence[LeafGen], consts: np.ndarray, prog_seed: int,
                    pin_rows: np.ndarray, pin_mask: np.ndarray, seed: int, first_index: int,
                    lanes: int, lane0: int = 0, n_lanes: Optional[int] = None,
                    want_classes: bool = False):
    """Host-only: lanes ``lane0 .. lane0 + n_lanes - 1`` of one mg_carry_batch
    job as the fill kernel writes them (mg_carry_fill_host, the kernel's own
    lane function): ``(n_leaves, 8, n_lanes)`` uint32, and with
    ``want_classes`` the generator branch of every free leaf and lane
    (0 r0, 1 boundary, 2 pool, 3 uniform; 0xFFFFFFFF: pinned)."""
    lib = load_library(check_digest=False)
    gens = list(leafgen)
    n = len(gens)
    n_lanes = lanes - lane0 if n_lanes is None else n_lanes
    garr = (LeafGen * max(1, n))(*gens)
    consts = np.ascontiguousarray(consts, dtype=np.uint32).reshape(-1, 8)
    rows = np.ascontiguousarray(pin_rows, dtype=np.uint32).reshape(-1, 8)
    mask = np.ascontiguousarray(pin_mask, dtype=np.uint32).reshape(-1)
    if rows.shape[0] != n or mask.shape[0] != (n + 31) // 32:
        raise ValueError("pin rows must be (n_leaves, 8) and the pin mask (n_leaves + 31) // 32 "
                         "words")
    out = np.zeros((n, 8, max(0, n_lanes)), dtype=np.uint32)
    cls = np.zeros((n, max(0, n_lanes)), dtype=np.uint32) if want_classes else None
    rc = lib.mg_carry_fill_host(C.cast(garr, C.c_void_p), n, _ptr(consts), consts.shape[0],
                                prog_seed & (2**64 - 1), _ptr(rows), _ptr(mask),
                                seed & (2**64 - 1), first_index, lanes, lane0, max(0, n_lanes),
                                _ptr(out), _ptr(cls))
    if rc != 0:
        raise EngineError("mg_carry_fill_host refused its arguments (%d)" % rc)
    return (out, cls) if want_classes else out


def carry_ladder_plan_host(n_leaves: Sequence[int], n_rungs: Sequence[int], lanes: int,
                           max_leaves: int):
    """Host-only: :func:`carry_plan_host` for mg_carry_ladder
    (mg_carry_ladder_plan_host): the same regions under the same indices, a
    job's mask region holding its ``n_rungs`` masks and every leaf region the
    largest ``n_rungs`` x ``lanes`` columns.  :class:`EngineError` where the
    library refuses: counts out of range, more than 2^20 columns or sizes
    beyond 64 bits."""
    lib = load_library(check_digest=False)
    counts = np.ascontiguousarray(n_leaves, dtype=np.uint32)
    rungs = np.ascontiguousarray(n_rungs, dtype=np.uint32)
    n = counts.shape[0]
    if rungs.shape[0] != n:
        raise ValueError("one n_rungs per job")
    offs = np.zeros(CARRY_SHARED + max(1, n) * CARRY_JOB_REGIONS, dtype=np.uint64)
    total, stride = C.c_uint64(0), C.c_uint64(0)
    rc = lib.mg_carry_ladder_plan_host(_ptr(counts), _ptr(rungs), n, lanes, max_leaves,
                                       _ptr(offs), C.byref(total), C.byref(stride))
    if rc != 0:
        raise EngineError("carry_ladder: %d jobs at %d lanes: counts out of range, too many "
                          "columns or a buffer beyond 64 bits" % (n, lanes))
    return offs[:CARRY_SHARED + n * CARRY_JOB_REGIONS], int(total.value), int(stride.value)


def carry_census_plan_host(n_leaves: Sequence[int], n_rungs: Sequence[int],
                           n_roots: Sequence[int], n_probes: Sequence[int],
                           mask_probe0: Sequence[int], lanes: int, walkers: int, max_leaves: int):
    """Host-only: the plan of mg_carry_census's device buffer
    (mg_carry_census_plan_host): ``(offsets, bytes, leaf_stride_w,
    probe_stride_w)``.  ``offsets``: :func:`carry_ladder_plan_host`'s table
    followed by the census records' offset and per job its counter blocks' and
    its probe region's.  :class:`EngineError` where the library refuses."""
    lib = load_library(check_digest=False)
    arrs = [np.ascontiguousarray(a, dtype=np.uint32)
            for a in (n_leaves, n_rungs, n_roots, n_probes, mask_probe0)]
    n = arrs[0].shape[0]
    if any(a.shape[0] != n for a in arrs):
        raise ValueError("one count of each kind per job")
    size = CARRY_SHARED + CARRY_CENSUS_SHARED + n * (CARRY_JOB_REGIONS + CARRY_CENSUS_JOB_REGIONS)
    offs = np.zeros(size + CARRY_JOB_REGIONS + CARRY_CENSUS_JOB_REGIONS, dtype=np.uint64)
    total, stride, pstride = C.c_uint64(0), C.c_uint64(0), C.c_uint64(0)
    rc = lib.mg_carry_census_plan_host(*[_ptr(a) for a in arrs], n, lanes, walkers, max_leaves,
                                       _ptr(offs), C.byref(total), C.byref(stride),
                                       C.byref(pstride))
    if rc != 0:
        raise EngineError("carry_census: %d jobs at %d lanes and %d walkers: counts out of range, "
                          "too many columns, mask probes outside the program's or a buffer "
                          "beyond 64 bits" % (n, lanes, walkers))
    return offs[:size], int(total.value), int(stride.value), int(pstride.value)


def carry_starts_host(blocks: np.ndarray, n_roots: int, walkers: int):
    """Host-only: the start rule (mg_carry_starts_host) on one job's counter
    blocks ``(n_rungs, 5 * n_roots + 2)`` uint64 (``census.pack_block`` of each
    rung's census): ``(start_col, start_nfail)``."""
    lib = load_library(check_digest=False)
    blocks = np.ascontiguousarray(blocks, dtype=np.uint64)
    if blocks.ndim != 2 or blocks.shape[1] != 5 * n_roots + 2:
        raise ValueError("counter blocks must be (n_rungs, 5 * n_roots + 2)")
    col = np.full(max(1, walkers), -1, dtype=np.int64)
    nfail = np.zeros(max(1, walkers), dtype=np.uint32)
    rc = lib.mg_carry_starts_host(_ptr(blocks), n_roots, blocks.shape[0], walkers, _ptr(col),
                                  _ptr(nfail))
    if rc != 0:
        raise EngineError("mg_carry_starts_host refused its arguments (%d)" % rc)
    return col, nfail


def carry_fill_rungs_host(leafgen: Sequence[LeafGen], consts: np.ndarray, prog_seed: int,
                          pin_rows: np.ndarray, pin_masks: np.ndarray, seed: int,
                          first_index: int, lanes: int, cols: Optional[int] = None, col0: int = 0,
                          n_cols: Optional[int] = None):
    """Host-only: columns ``col0 .. col0 + n_cols - 1`` of one mg_carry_ladder
    job as the rung fill kernel writes them (mg_carry_fill_rungs_host, the
    kernel's own lane function): ``(n_leaves, 8, n_cols)`` uint32.  ``cols``:
    the job's columns in its batch (default: its own ``n_rungs * lanes``)."""
    lib = load_library(check_digest=False)
    gens = list(leafgen)
    n = len(gens)
    garr = (LeafGen * max(1, n))(*gens)
    consts = np.ascontiguousarray(consts, dtype=np.uint32).reshape(-1, 8)
    rows = np.ascontiguousarray(pin_rows, dtype=np.uint32).reshape(-1, 8)
    masks = np.ascontiguousarray(pin_masks, dtype=np.uint32)
    if rows.shape[0] != n or masks.ndim != 2 or masks.shape[1] != (n + 31) // 32:
        raise ValueError("pin rows must be (n_leaves, 8) and the pin masks (n_rungs, "
                         "(n_leaves + 31) // 32)")
    cols = masks.shape[0] * lanes if cols is None else cols
    n_cols = cols - col0 if n_cols is None else n_cols
    out = np.zeros((n, 8, max(0, n_cols)), dtype=np.uint32)
    rc = lib.mg_carry_fill_rungs_host(C.cast(garr, C.c_void_p), n, _ptr(consts), consts.shape[0],
                                      prog_seed & (2**64 - 1), _ptr(rows), _ptr(masks),
                                      masks.shape[0], seed & (2**64 - 1), first_index, lanes, cols,
                                      col0, max(0, n_cols), _ptr(out))
    if rc != 0:
        raise EngineError("mg_carry_fill_rungs_host refused its arguments (%d)" % rc)
    return out


def carry_sets_plan_host(n_leaves: Sequence[int], n_rungs: Sequence[int], n_sets: Sequence[int],
                         lanes: int, max_leaves: int):
    """Host-only: the plan of mg_carry_ladder_sets's device buffer
    (mg_carry_sets_plan_host): ``(offsets, bytes, leaf_stride_w)``.
    ``offsets``: :func:`carry_ladder_plan_host`'s table — a job's rows region
    holding its ``n_sets`` row sets — followed by the set records' offset and
    per job its rung_set's.  :class:`EngineError` where the library refuses."""
    lib = load_library(check_digest=False)
    arrs = [np.ascontiguousarray(a, dtype=np.uint32) for a in (n_leaves, n_rungs, n_sets)]
    n = arrs[0].shape[0]
    if any(a.shape[0] != n for a in arrs):
        raise ValueError("one count of each kind per job")
    size = CARRY_SHARED + CARRY_SETS_SHARED + n * (CARRY_JOB_REGIONS + CARRY_SETS_JOB_REGIONS)
    offs = np.zeros(size + CARRY_JOB_REGIONS + CARRY_SETS_JOB_REGIONS, dtype=np.uint64)
    total, stride = C.c_uint64(0), C.c_uint64(0)
    rc = lib.mg_carry_sets_plan_host(*[_ptr(a) for a in arrs], n, lanes, max_leaves, _ptr(offs),
                                     C.byref(total), C.byref(stride))
    if rc != 0:
        raise EngineError("carry_sets: %d jobs at %d lanes: counts out of range, too many "
                          "columns or a buffer beyond 64 bits" % (n, lanes))
    return offs[:size], int(total.value), int(stride.value)


def carry_fill_sets_host(leafgen: Sequence[LeafGen], consts: np.ndarray, prog_seed: int,
                         pin_rows: np.ndarray, pin_masks: np.ndarray, rung_set: np.ndarray,
                         seed: int, first_index: int, lanes: int, cols: Optional[int] = None,
                         col0: int = 0, n_cols: Optional[int] = None):
    """Host-only: :func:`carry_fill_rungs_host` for one mg_carry_ladder_sets
    job (mg_carry_fill_sets_host, the set fill kernel's own lane function):
    ``pin_rows`` ``(n_sets, n_leaves, 8)``, ``rung_set`` ``(n_rungs,)``."""
    lib = load_library(check_digest=False)
    gens = list(leafgen)
    n = len(gens)
    garr = (LeafGen * max(1, n))(*gens)
    consts = np.ascontiguousarray(consts, dtype=np.uint32).reshape(-1, 8)
    rows = np.ascontiguousarray(pin_rows, dtype=np.uint32)
    masks = np.ascontiguousarray(pin_masks, dtype=np.uint32)
    sets = np.ascontiguousarray(rung_set, dtype=np.uint32)
    if rows.ndim != 3 or rows.shape[1:] != (n, 8) or masks.ndim != 2 or \
            masks.shape[1] != (n + 31) // 32 or sets.shape != (masks.shape[0],):
        raise ValueError("pin rows must be (n_sets, n_leaves, 8), the pin masks (n_rungs, "
                         "(n_leaves + 31) // 32) and rung_set (n_rungs,)")
    cols = masks.shape[0] * lanes if cols is None else cols
    n_cols = cols - col0 if n_cols is None else n_cols
    out = np.zeros((n, 8, max(0, n_cols)), dtype=np.uint32)
    rc = lib.mg_carry_fill_sets_host(C.cast(garr, C.c_void_p), n, _ptr(consts), consts.shape[0],
                                     prog_seed & (2**64 - 1), _ptr(rows), _ptr(masks), _ptr(sets),
                                     masks.shape[0], rows.shape[0], seed & (2**64 - 1),
                                     first_index, lanes, cols, col0, max(0, n_cols), _ptr(out))
    if rc != 0:
        raise EngineError("mg_carry_fill_sets_host refused its arguments (%d)" % rc)
    return out


def census_batch_blocks_host(n_jobs: int, n: int) -> int:
    """Host-only: blocks per job of one mg_census_batch_kernel launch over
    ``n`` candidates (mg_census_batch_blocks_host)."""
    return int(load_library(check_digest=False).mg_census_batch_blocks_host(n_jobs, n))


def split_census_jobs(shapes: Sequence[CensusShape], max_jobs: int = CENSUS_BATCH_MAX_JOBS):
    """Consecutive ``(lo, hi)`` ranges that cover ``shapes`` once, in order,
    each the longest run from its start that stays within ``max_jobs`` and
    whose probe regions fit the library's probe buffer at 256 candidates per
    chunk, the smallest chunk there is (with chunk 0 the library then chooses
    the largest that fits).  A run of one job is always tried: what is wrong
    with it alone, the library says."""
    lib = load_library(check_digest=False)
    offs = np.zeros(CENSUS_BATCH_SHARED + max_jobs * CENSUS_BATCH_JOB_REGIONS, dtype=np.uint64)
    total, got = C.c_uint64(0), C.c_uint64(0)

    def fits(lo, hi):
        arr = (CensusShape * (hi - lo))(*shapes[lo:hi])
        return lib.mg_census_batch_plan_host(arr, hi - lo, 256, 256, _ptr(offs), C.byref(total),
                                             C.byref(got), None, 0) == 0
    parts, lo, n = [], 0, len(shapes)
    while lo < n:
        hi = lo + 1
        while hi < n and hi - lo < max_jobs and fits(lo, hi + 1):
            hi += 1
        parts.append((lo, hi))
        lo = hi
    return parts


def _uf_arrays(ufs):
    """The UF tables of ``repair.Ufs`` as contiguous u32 arrays (slots (n, 2),
    funcs (f, 3), cands (c, 6), ukeys (k, 8))."""
    tabs = tuple(np.ascontiguousarray(a, dtype=np.uint32)
                 for a in (ufs.slots, ufs.funcs, ufs.cands, ufs.ukeys))
    if [a.shape[1:] for a in tabs] != [(2,), (3,), (6,), (8,)]:
        raise ValueError("ufs.slots must be (n, 2), ufs.funcs (f, 3), ufs.cands (c, 6), "
                         "ufs.ukeys (k, 8)")
    return tabs


def _uf_args(tabs):
    """(pointer or None, rows) per table, as the C ABI takes them."""
    out = []
    for a in tabs:
        out += [_ptr(a) if a.size else None, a.shape[0]]
    return out


def walk_uf_resolve_host(leafgen: Sequence[LeafGen], base: np.ndarray, urows: np.ndarray, ufs):
    """Host-only (no GPU): the destinations (n_slots,) u32 of the slots of
    ``ufs`` under ``base`` (n_leaves, 8) and the U rows ``urows`` (n_urows, 8)
    from the library's own resolver (mg_walk_uf_resolve_host;
    ``repair.uf_resolve_ref`` is its specification)."""
    lib = load_library()
    gens = list(leafgen)
    garr = (LeafGen * max(1, len(gens)))(*gens)
    base = np.ascontiguousarray(base, dtype=np.uint32)
    urows = np.ascontiguousarray(urows, dtype=np.uint32).reshape(-1, 8)
    tabs = _uf_arrays(ufs)
    if urows.shape[0] < ufs.n_urows:
        raise EngineError("mg_walk_uf_resolve_host: urows shorter than n_urows")
    dest = np.zeros(max(1, tabs[0].shape[0]), dtype=np.uint32)
    rc = lib.mg_walk_uf_resolve_host(C.cast(garr, C.c_void_p), len(gens), _ptr(base),
                                     _ptr(urows) if urows.size else None, int(ufs.n_urows),
                                     *_uf_args(tabs), _ptr(dest))
    if rc != 0:
        raise EngineError("mg_walk_uf_resolve_host failed (%d)" % rc)
    return dest[:tabs[0].shape[0]]


def walk_uf_mutate_host(leafgen: Sequence[LeafGen], consts: np.ndarray, base: np.ndarray,
                        state, bounds, ufs, seed: int, r: int, lanes: int, lane0: int = 0,
                        n_lanes: Optional[int] = None, n_resid: Optional[int] = None):
    """Host-only (no GPU): :func:`walk_bound_mutate_host` for the lane function
    of mg_walk_uf (mg_walk_uf_mutate_host; ``repair.uf_mutate_ref`` is its
    specification).  ``state``: ``(rvals, root bits, atom bits, dest (n_slots,)
    u32)``, None in round 0."""
    return _walk_mutate_host("mg_walk_uf_mutate_host", leafgen, consts, base, state, bounds, ufs,
                             None, seed, r, lanes, lane0, n_lanes, n_resid)


def walk_sum_mutate_host(leafgen: Sequence[LeafGen], consts: np.ndarray, base: np.ndarray,
                         state, bounds, ufs, sums, seed: int, r: int, lanes: int, lane0: int = 0,
                         n_lanes: Optional[int] = None, n_resid: Optional[int] = None):
    """Host-only (no GPU): :func:`walk_uf_mutate_host` for the lane function
    of mg_walk_sum (mg_walk_sum_mutate_host; ``repair.sum_mutate_ref`` is its
    specification).  ``state``: ``(rvals, root bits, atom bits, dest (n_slots,)
    u32, srows (n_srows, 8) u32)``, None in round 0."""
    return _walk_mutate_host("mg_walk_sum_mutate_host", leafgen, consts, base, state, bounds, ufs,
                             sums, seed, r, lanes, lane0, n_lanes, n_resid)


def walk_score_host(masks: np.ndarray, resid: Optional[np.ndarray], table: np.ndarray,
                    n_roots: int):
    """Host-only (no GPU): ``(nfail, cost)`` (n,) u32 of the lanes of mask
    probes ``masks`` (n_mask, 8, n) u32 and residual probes ``resid``
    (n_resid, 8, n) u32 from the library's own scoring function
    (mg_walk_score_host; ``repair.score_ref`` is its specification)."""
    lib = load_library()
    masks = np.ascontiguousarray(masks, dtype=np.uint32)
    n = masks.shape[2]
    n_resid = 0 if resid is None else resid.shape[0]
    resid = None if not n_resid else np.ascontiguousarray(resid, dtype=np.uint32)
    table = np.ascontiguousarray(table, dtype=np.uint32)
    nfail, cost = np.zeros(max(1, n), dtype=np.uint32), np.zeros(max(1, n), dtype=np.uint32)
    rc = lib.mg_walk_score_host(_ptr(masks), _ptr(resid), _ptr(table), n_roots, n_resid, n,
                                _ptr(nfail), _ptr(cost))
    if rc != 0:
        raise EngineError("mg_walk_score_host failed (%d)" % rc)
    return nfail[:n], cost[:n]


def walk_tree_score_host(masks: np.ndarray, amasks: Optional[np.ndarray],
                         resid: Optional[np.ndarray], trees, n_roots: int,
                         n_resid: Optional[int] = None):
    """Host-only (no GPU): ``(nfail, cost)`` (n,) u32 of the lanes of root-mask
    probes ``masks``, atom-mask probes ``amasks`` and residual probes
    ``resid`` (each (.., 8, n) u32) from the library's own tree scoring
    (mg_walk_tree_score_host; ``repair.tree_score_ref`` is its specification);
    ``trees``: roots, atoms and code (``repair.Trees``)."""
    lib = load_library()
    masks = np.ascontiguousarray(masks, dtype=np.uint32)
    n = masks.shape[2]
    have = 0 if resid is None else resid.shape[0]
    n_resid = have if n_resid is None else n_resid
    resid = None if not have else np.ascontiguousarray(resid, dtype=np.uint32)
    roots = np.ascontiguousarray(trees.roots, dtype=np.uint32)
    atoms = np.ascontiguousarray(trees.atoms, dtype=np.uint32)
    code = np.ascontiguousarray(trees.code, dtype=np.uint32)
    if atoms.size:
        amasks = np.ascontiguousarray(amasks, dtype=np.uint32)
        if amasks.ndim != 3 or amasks.shape[1:] != (8, n) or amasks.shape[0] * 256 < atoms.size:
            raise ValueError("amasks must be (ceil(n_atoms / 256), 8, n)")
    if roots.size < n_roots or masks.shape[0] * 256 < n_roots or (
            have and resid.shape[1:] != (8, n)) or n_resid > have:
        raise EngineError("mg_walk_tree_score_host: tables or rows shorter than n_roots, n_resid")
    nfail, cost = np.zeros(max(1, n), dtype=np.uint32), np.zeros(max(1, n), dtype=np.uint32)
    rc = lib.mg_walk_tree_score_host(_ptr(masks), _ptr(amasks) if atoms.size else None,
                                     _ptr(resid), _ptr(roots) if roots.size else None, n_roots,
                                     _ptr(atoms) if atoms.size else None, atoms.size,
                                     _ptr(code) if code.size else None, code.size, n_resid, n,
                                     _ptr(nfail), _ptr(cost))
    if rc != 0:
        raise EngineError("mg_walk_tree_score_host failed (%d)" % rc)
    return nfail[:n], cost[:n]


def unpack_bits(bits: np.ndarray, n: int) -> np.ndarray:
    b = np.unpackbits(bits.view(np.uint8), bitorder="little")
    return b[:n].astype(bool)


def int_to_limbs(v: int) -> List[int]:
    return [(v >> (32 * j)) & 0xFFFFFFFF for j in range(8)]


def limbs_to_int(limbs) -> int:
    v = 0
    for j in reversed(range(8)):
        v = (v << 32) | int(limbs[j])
    return v


_engines: Dict[Tuple[int, int, int], Engine] = {}
_failed: Dict[Tuple[int, int], str] = {}
_engines_lock = threading.Lock()


def get_engine(device: int = 0, slot: int = 0, nreg: Optional[int] = None) -> Engine:
    """The engine (one HIP context) of ``device`` running the ``nreg``-slot
    register layout (default: the process's); ``slot`` > 0 gives further
    independent contexts on the same device (a device listed twice in
    ``MYTHRIL_GPU_DEVICES`` is searched from two host threads, and a context
    serves one thread at a time).  An initialisation failure is remembered
    per (device, slot), so later calls raise EngineUnavailable at once
    instead of retrying mg_init; a failed extra slot (e.g. out of memory for
    one more context) does not mark the device's first context failed, and
    the exception carries ``slot`` so callers can tell the two apart."""
    from . import irdefs
    nreg = irdefs.NREG if nreg is None else int(nreg)
    with _engines_lock:
        e = _engines.get((device, slot, nreg))
        if e is None:
            for key in ((device, 0), (device, slot)):
                if key in _failed:
                    raise EngineUnavailable(_failed[key], slot=key[1], device=device)
            try:
                e = Engine(device, nreg=nreg)
            except EngineUnavailable as x:
                _failed[(device, slot)] = str(x)
                raise EngineUnavailable(str(x), slot=slot, device=device) from x
            except Exception as x:  # noqa: BLE001 - any init failure means no engine
                _failed[(device, slot)] = "%s: %s" % (type(x).__name__, x)
                raise EngineUnavailable(_failed[(device, slot)], slot=slot, device=device) from x
            _engines[(device, slot, nreg)] = e
        return e


def device_slots(devices) -> List[Tuple[int, int]]:
    """(device, slot) per entry of a device list: the k-th repeat of a device
    gets slot k, its own context."""
    seen: Dict[int, int] = {}
    out = []
    for d in devices:
        out.append((d, seen.get(d, 0)))
        seen[d] = seen.get(d, 0) + 1
    return out
