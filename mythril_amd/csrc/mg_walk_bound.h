/* The aimed moves of mg_walk_bound, for host and device:
 * the lane function of mg_walk_aim.h with a wider aim table, whose entries
 * are the XOR entries of §3.12 or order entries.  This header describes the
 * tables; the code is that of mg_walk_sum.h, which nests this rung
 * (mg_walk_bound_lane, mg_walk_bound_ok and mg_walk_bound_live are its lane
 * function, validator and live rule with no lin word, no UF table and no
 * destination).  The kernels of mg_walk_sum.hip and the host entry the CPU
 * suite compares with the specification (mg_walk_bound_mutate_host) run that
 * code.  Specification, bit for bit: mythril_amd/repair.py bound_mutate_ref.
 *
 * An order atom lo < hi / lo <= hi carries the residual probe D = lo - hi.
 * Where side lo is made of leaves, lo - D - s = hi - s (s = 1 for the strict
 * orders) makes the order hold in one move; where hi is, hi + D + s = lo + s.
 *   entries[5 e ..]  residual probe, first piece, pieces (1 .. 64), mode, truth
 *   pieces[4 p ..]   leaf, leaf_bit, value_bit, len
 *   fixed[8 e ..]    the side's numeral bits (a numeral operand of a concat)
 *   mode             0 XOR, 1 LOW, 2 LOW_STRICT, 3 HIGH, 4 HIGH_STRICT
 *   truth            1 << 31 | i: bit i of the atom mask; else bit k of the
 *                    root mask (XOR entries: 0, and fixed is 0)
 * An order entry gathers the side's value from the base,
 *   V = fixed | OR over pieces ((base[leaf] >> leaf_bit) & mask(len)) << value_bit
 * takes T = V - D - s (LOW) or V + D + s (HIGH) mod 2^256, and scatters it in
 * piece order into the lane's current value of each leaf:
 *   leaf = leaf & ~(mask(len) << leaf_bit) | ((T >> value_bit) & mask(len)) << leaf_bit
 * Bits at or above the side's width are never scattered and carries only go
 * upward, so no width is needed.
 *
 * L = the live entries in table order (empty in round 0): an XOR entry is
 * live iff its residual is not 0 under the base, an order entry iff its truth
 * bit is clear on the base.  The mask state of a base is its root-mask rows,
 * then its atom-mask rows: mask bit k is bit k % 32 of word k / 32.  The lane
 * layout is mg_walk_aim's exactly (mg_walk_aim_pick). */
#ifndef MG_WALK_BOUND_H
#define MG_WALK_BOUND_H

#include <stdint.h>
#include "mg_walk_sum.h"

#endif
