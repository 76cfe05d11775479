/* raftx_mooring.h -- quasi-static mooring lines of rigid 6-DOF designs at a given pose (libraftx_hip.so only).
 *
 * Replaces, per unit, what the reference does with a MoorPy system for moorMod == 0 and lines that are ONE catenary
 * segment from a fixed anchor to a point on the vessel:
 *     raft_fowt.py:799-808     ms.solveEquilibrium (no free points: every line is solved on its own),
 *                              C_moor = ms.getCoupledStiffnessA, F_moor = ms.getForces
 *     raft_fowt.py:2356-2373   the tension Jacobian J_moor and the mean tensions T_moor (ends A, then ends B)
 * at the pose the caller gives.  The mean-pose solve (Model.solveStatics) is not part of it.
 *
 * Line record (RAFTX_ML_N doubles):
 *     0-2   anchor, global coordinates
 *     3-5   fairlead in the body frame, relative to the unit's reference point
 *     6     unstretched length L            7   EA            8   w, submerged weight per length
 *     9     seabed friction CB: must be 0 (refused otherwise; friction is not covered)
 *     10-15 zero
 * A COMPOSITE line -- segments in series, joined at free points that may carry a clump weight or a buoy (MoorPy: one Line
 * per segment between points of type free) -- occupies consecutive rows, ordered anchor -> fairlead; nLine counts rows,
 * that is segments, everywhere.  Its head row is the record above with the anchor-side segment's L, EA, w.  Each further
 * segment is a CONTINUATION row:
 *     15 (RAFTX_ML_CONT)   1
 *     6-8                  its own L, EA, w            9   CB, must be 0
 *     10 (RAFTX_ML_WJOINT) net submerged weight [N] of the point at its lower end, (m - rho v) g: negative for a buoy,
 *                          0 for a plain joint
 *     0-5, 11-14           zero
 * At most RAFTX_MOOR_MAX_SEG rows per line.  A row with field 15 equal to 0 that no continuation row follows is a single line
 * and takes the arithmetic, and gives the bits, of a batch without composite lines.  On a frictionless seabed HF is the same
 * in every segment and V at the top of a segment is VF less the segments and points hanging above it, so the chain is
 * solved for the fairlead's (HF, VF) like a single line, with the summed span and Jacobian; the guess uses the total length
 * and the mean weight per length (which must be positive).  Only the anchor-side segment may rest on the seabed.
 * C_moor and F_moor receive a chain once (from its head row); T and J have the two ends of every row, in the order of
 * getTensions for a system with one Line per segment.  line_out of a continuation row: HF, V at its top, HF, V at its bottom,
 * 0, the chain's iterations, 0; of a head row: its own segment's, L_B and the branch included.
 * The fairlead is at x[0:3] + R(x[3:6]) r_f, R = Rz Ry Rx of (roll, pitch, yaw): the rotation of the member descriptors.
 * The elastic catenary (no seabed contact, or partly resting on a frictionless seabed when the anchor lies on it,
 * |a_z + depth| <= 1e-6 depth) is solved for the fairlead's (HF, VF) by a damped Newton iteration to stagnation in fp64,
 * at most 60 steps.  C_moor = -dF_moor/dx6 is the exact derivative for a translation and an infinitesimal rotation
 * vector about the reference point applied on top of R; it includes the arm turning under a fixed force and is not
 * symmetric in general.  J = dT/dx6 in the same sense.
 *
 * Flags (int32 per design; a flagged design's outputs are NaN, and only its own).  For a composite line BAD_LINE looks at
 * the L, EA, w of every row (segments must be heavier than water: buoyancy enters through the points only), SLACK and
 * VERTICAL at the total length.
 *
 * A BRIDLE (crowfoot, delta connection) -- a stem from the anchor to a free junction, and 2 .. RAFTX_MOOR_MAX_LEG legs from the
 * junction to fairleads of their own -- occupies consecutive rows too:
 *     stem rows   the head row and its continuation rows exactly as above (anchor -> junction), at most RAFTX_MOOR_MAX_SEG; the
 *                 head row's fields 3-5 must be zero: the stem ends at the junction, not on the vessel
 *     leg rows    14 (RAFTX_ML_LEG) 1, 15 zero; 3-5 the leg's fairlead in the body frame; 6-8 its own L, EA, w; 9 CB, must be 0;
 *                 10 (RAFTX_ML_WJOINT) on the FIRST leg row the junction's net submerged weight [N] (negative for a buoy), 0 on
 *                 the others; every other field zero
 * The junction's three coordinates are the unknowns of a damped Newton iteration (at most 60 steps, to stagnation) on the sum
 * of the stem's end force, every leg's lower-end force (a leg is one suspended catenary: it never rests on the seabed) and the
 * junction weight.  C_moor is the stiffness condensed to the fairleads, over all pairs of legs -- the fairleads are coupled
 * through the junction -- with the arm-turning term of every fairlead; J of every row end includes the junction's motion.
 * T and J keep their layout (a leg's end A is at the junction, its end B at its fairlead); C_moor and F_moor receive a bridle
 * once; line_out of a leg row: HF, V at its top, HF, V at its bottom, 0, the junction iteration's steps, 0, 0 (the stem rows
 * hold the junction iteration's steps in field 5 as well).  A batch without a leg row takes the code path, the kernels and the
 * bits of a library without bridles.  Flags of a bridle: BAD_LINE as for a composite line, over all its rows (and a fairlead
 * not above the anchor); SLACK when L_stem + L_leg >= XF + ZF from the anchor to the leg's fairlead holds for EVERY leg;
 * GROUNDED by the composite line's rule for the stem, or the junction or the sag of a leg more than 1e-6 depth below the
 * seabed; NO_CONVERGENCE when the junction iteration reaches its cap or finds no admissible start.
 * Every entry point that takes line records takes bridles: raftx_mooring_lines, raftx_mooring_program, raftx_mean_pose
 * (include/raftx_statics.h), raftx_sweep_mooring and raftx_sweep_mean_pose.
 * Still refused: lines with both ends on ONE vessel (a line from one unit of an array to another is a shared row of
 * include/raftx_array_mooring.h), shared anchors, junctions joined to junctions, seabed friction, the fully
 * slack profile, seabed contact of any segment but the anchor-side one.
 */
#ifndef RAFTX_MOORING_H
#define RAFTX_MOORING_H

#include "raftx.h"

#define RAFTX_ML_N 16
#define RAFTX_ML_WJOINT 10             /* continuation row: net submerged weight of the point at its lower end */
#define RAFTX_ML_LEG 14                /* 1 in a leg row of a bridle (field 15 is 0 there), 0 in every other row */
#define RAFTX_ML_CONT 15               /* 1 in a continuation row of a composite line, 0 in a head row or a single line */
#define RAFTX_MOOR_MAX_SEG 4           /* rows of one composite line, or stem rows of one bridle, at most */
#define RAFTX_MOOR_MAX_LEG 3           /* leg rows of one bridle, at most (and at least 2) */
#define RAFTX_MOOR_BAD_LINE        1   /* non-finite field or pose; L, EA or w <= 0; anchor below the seabed; fairlead not above the anchor */
#define RAFTX_MOOR_VERTICAL        2   /* horizontal span XF <= 1e-9 L */
#define RAFTX_MOOR_SLACK           4   /* L >= XF + ZF: the fully slack profile is not covered */
#define RAFTX_MOOR_NO_CONVERGENCE  8   /* the Newton cap was reached */
/* (16 and 32 are the flags of raftx_statics.h) */
#define RAFTX_MOOR_GROUNDED       64   /* composite line: the anchor-side segment rests wholly on the seabed (V at its top <= 0), or a
                                          joint or the sag of a segment lies more than 1e-6 depth below the seabed */

#ifdef __cplusplus
extern "C" {
#endif

/* Stateless (raft_fowt.py:799-808 and :2356-2373 for every design at once).  lines [nDesign,nLine,RAFTX_ML_N],
 * pose [nDesign,6] (m, rad) or NULL (zero), depth > 0.  Outputs, each of which may be NULL except flags:
 * C_moor [nDesign,6,6], F_moor [nDesign,6], T [nDesign,2 nLine] (ends A of all lines, then ends B: the order of
 * getTensions), J [nDesign,2 nLine,6], line_out [nDesign,nLine,8] = HF, VF, HA, VA, L_B, iterations, branch
 * (1 = seabed contact), 0, flags [nDesign].  The sums over the lines run in line order without atomics: the bits of a
 * design depend on its own lines and pose only.  Errors, before any launch: nLine < 1, nDesign < 0, NULL lines or flags,
 * a depth that is not positive and finite, a line with CB != 0, a design whose row 0 is a continuation row, a composite
 * line of more than RAFTX_MOOR_MAX_SEG rows; a leg row that follows no head row, a bridle of one leg or of more than
 * RAFTX_MOOR_MAX_LEG, a non-zero fairlead on the head row of a bridle, a row with both marks. */
int raftx_mooring_lines(raftx_ctx *ctx, int nDesign, int nLine, const double *lines, const double *pose, double depth,
                        double *C_moor, double *F_moor, double *T, double *J, double *line_out, int32_t *flags);

/* The mooring edits of a parametric sweep (raft/parametersweep.py:64-68, 79-83: the fairleads follow the outer
 * columns): base records lines [nLine,RAFTX_ML_N] and, for lines with lineEdit != 0, anchor and fairlead coordinates
 * (fields 0-5) that are affine in the variant parameters, lineCoef [nLine,6,nParam+1] = constant, then one coefficient
 * per parameter, evaluated left to right without fused multiply-adds exactly as endCoef of raftx_variant_program.
 * nParam must equal the installed variant program's (an error without one).  nLine = 0 clears the program; installing a
 * new variant program does not.  Continuation rows are carried unchanged to every variant; a lineEdit on one is an error
 * (the anchor and the fairlead of a composite line are its head row's), as are the record errors of raftx_mooring_lines.
 * A lineEdit on a leg row of a bridle may move its fairlead only (fields 3-5), on the head row of a bridle its anchor only
 * (fields 0-2): a non-zero coefficient for one of the other three fields is an error. */
int raftx_mooring_program(raftx_ctx *ctx, int nLine, const double *lines, int nParam, const double *lineCoef,
                          const int32_t *lineEdit);

/* The line records lines_out [nDesign,nLine,RAFTX_ML_N] of the variants params [nDesign,nParam], written by the device and
 * copied back: for checks. */
int raftx_mooring_expand(raftx_ctx *ctx, int nDesign, const double *params, double *lines_out);

/* On a PREPARED, not yet launched sweep slot (raftx_sweep_prepare / raftx_sweep_prepare_variants), as raftx_sweep_modal: the
 * mooring system of every design of the crossing (raft_fowt.py:799-808, 2356-2373) at the crossing's pose and depth.
 * lines [nDesign,nLine,RAFTX_ML_N], or NULL on a raftx_sweep_prepare_variants slot: the records of the installed mooring
 * program fed the slot's params (nLine must be the program's).  The kernels run at once on the copy stream, before the
 * crossing is launched.
 * add_stiffness != 0: every block's device C0 receives += C_moor after its upload and before anything reads it (k_geom_addup,
 * the add-up inside k_geom_design and the generating fused kernel all wait for it): the crossing is the one a caller would
 * get by passing C0 + C_moor, bit for bit.  A flagged design's C_moor is NaN: its pairs' responses are not finite, nobody
 * else's.
 * T_std [nDesign,nCase,2 nLine] or NULL: the standard deviations of J Xi (raft_fowt.py:2367-2371), by a second launch of
 * k_sweep_channels per block on rows the mooring kernel left in device memory; a raftx_sweep_channels request on the same
 * slot is not disturbed.  C_moor [nDesign,6,6], F_moor [nDesign,6], T_mean [nDesign,2 nLine] may be NULL; flags [nDesign]
 * is required.  Results land in a page-locked area and raftx_sweep_wait fills the caller's arrays (alive until then; the
 * inputs are copied).  A second request on a slot replaces the first; raftx_sweep_cancel and a new prepare drop it.
 * Errors, before any launch: an idle or launched slot; CB != 0; lines == NULL without a variant slot, without a mooring
 * program, or with another nLine / parameter count. */
int raftx_sweep_mooring(raftx_ctx *ctx, int slot, int nLine, const double *lines, int add_stiffness, double *C_moor,
                        double *F_moor, double *T_mean, double *T_std, int32_t *flags);

#ifdef __cplusplus
}
#endif

#endif /* RAFTX_MOORING_H */
