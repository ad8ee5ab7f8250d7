/* The aimed moves of mg_walk_uf, for host and device: the
 * lane function of mg_walk_bound.h whose pieces may name a UF slot instead of
 * a leaf.  This header describes the tables; the code is that of
 * mg_walk_sum.h, which nests this rung (mg_walk_uf_lane is its lane function
 * with no lin word).  The kernels of mg_walk_sum.hip, which also resolve the
 * slots at every adoption, and the host entries the CPU suite compares with
 * the specification (mg_walk_uf_mutate_host, mg_walk_uf_resolve_host) run that
 * code.
 * Specification, bit for bit: mythril_amd/repair.py uf_resolve_ref,
 * uf_mutate_ref.
 *
 * A slot is one application f(arg) of an uninterpreted function.  Its value
 * is whichever entry of f's model table arg hits under the current
 * assignment, so the leaf an aim writes is resolved per walker, at every
 * adoption, from the adopted base and the adopted lane's U rows (the probes
 * after the residuals: the arguments' chunks, then the computed keys of
 * argument-keyed entries):
 *   slots[2 u ..]   function, first U row of the argument (one per key chunk)
 *   funcs[3 f ..]   first candidate, candidates, key chunks (1 .. 4)
 *   cands[6 c ..]   value leaf or MG_AIM_NONE, key kind, key word per chunk
 *   ukeys[8 n ..]   the chunks of the constant keys
 *   key kind        0 CONST: a row of ukeys; 1 LEAF: a leaf; 2 PROBE: a U row;
 *                   3 ALWAYS: no key, matches (the else leaf)
 * The candidates of a function stand in the table's precedence order.  The
 * destination of slot u is the value leaf of the FIRST candidate of its
 * function all of whose key chunks equal the argument's U rows in all 8 limbs
 * (MG_AIM_NONE when none matches or that candidate has no value leaf).
 *
 *   pieces[4 p ..]  MG_UF_SLOT | u, leaf_bit, value_bit, len: acts on leaf
 *                   dest[u] wherever mg_walk_bound.h says leaf
 * An entry with a slot piece whose destination is MG_AIM_NONE is not live;
 * everything else (entries, fixed, modes, truth, L, the lane layout) is
 * mg_walk_bound.h's, and with no slot piece so is every neighbour. */
#ifndef MG_WALK_UF_H
#define MG_WALK_UF_H

#include <stdint.h>
#include "mg_walk_sum.h"

#endif
