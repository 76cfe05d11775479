/* raftx_qtfgen.h -- second-order slender-body QTF tables generated on the device (libraftx_hip.so only).
 *
 * raftx_qtf_slender (raftx.h) takes, per set, the strip / member records raft_amd/qtf.py pack_qtf makes of a reference
 * FOWT object (raft_member.py:1488-1674 reads mem.r, ds, drs, dls, ls and the Ca_* arrays).  The entries below make the
 * same records from the member / station descriptors raftx_build_designs takes (RAFTX_GM_*, RAFTX_GS_*), or from the
 * parameters of the installed raftx_variant_program, keep them resident, and run the QTF kernels on them with ONE table
 * per design for all its sea states:
 *
 *   strip record  RAFTX_QS_N = 24 doubles, one per strip node with z < 0 (raft_member.py:1553):
 *       0-2 r, 3-5 q, 6-8 p1, 9-11 p2 at the pose; 12 Ca_p1, 13 Ca_p2, 14 Ca_End at the strip (:1557-1559);
 *       15 v_side with the waterline scaling (:1562-1568); 16 v_end (:1613-1618); 17 a_i (:1343,1347);
 *       18 index of the member among the design's KEPT members; 19-23 zero
 *   member record RAFTX_QM_N = 16 doubles, one per member not wholly above water (:1493-1494):
 *       0 crosses-the-waterline flag, 1-3 r_int (:1523-1524); 4 waterline area (:1641-1657); 5-6 Ca_p1, Ca_p2 of the
 *       member's LAST submerged strip (:1660-1662); 7-9 p1; 10-12 p2; 13-15 zero
 *   Kim & Yue geometry, rows of RAFTX_QKG_N = 8 doubles, per member with RAFTX_GM_FLAG_MCF (circular, kept), in member
 *   order: two header rows
 *       [ns, rA(3), rB(3), first item of the member among the design's] [p1(3), p2(3), crosses flag, 0]
 *   then one row per strip node of the member, submerged or not: [r(3), ds, dls, 0, 0, 0]
 *   (what raft_amd/qtf.py kay_items reads: Member.correction_KAY, raft_member.py:1676-1791).
 * Order is member order, then strip order.  Caps play no part.  `beam` members are not covered.
 *
 * These prototypes are kept out of raftx.h on purpose: that header is the contract both the device library and the CPU
 * oracle implement, and the oracle has no counterpart.
 */
#ifndef RAFTX_QTFGEN_H
#define RAFTX_QTFGEN_H

#include "raftx.h"

#define RAFTX_QS_N 24
#define RAFTX_QM_N 16
#define RAFTX_QKG_N 8

#ifdef __cplusplus
extern "C" {
#endif

/* Generates the records of nDesign designs and leaves them resident on ctx until the next build or raftx_ctx_destroy;
 * independent of what raftx_upload_designs / raftx_build_designs left.  memberOff [nDesign+1], members
 * [nMember,RAFTX_GM_N], stationOff [nMember+1], stations [nStation,RAFTX_GS_N], pose [nDesign,6] or NULL: as
 * raftx_build_designs reads them.  stripOff_out / memOff_out [nDesign+1]: optional.  Errors (nothing is launched, the
 * tables of an earlier build are kept): missing arrays, offsets that are not monotone, a non-finite descriptor or pose.  A member with
 * fewer than two stations, dlsMax <= 0 or no length is reported after the counting pass; no tables are resident then. */
int raftx_qtf_tables_build(raftx_ctx *ctx, int nDesign, const int64_t *memberOff, const double *members,
                           const int64_t *stationOff, const double *stations, const double *pose, int64_t *stripOff_out,
                           int64_t *memOff_out);

/* The same for nDesign variants of the installed raftx_variant_program: params [nDesign,nParam] cross the bus, the
 * descriptors are written in device memory by the expansion kernel of raftx_sweep_prepare_variants.  An error without a
 * program. */
int raftx_qtf_tables_build_variants(raftx_ctx *ctx, int nDesign, const double *params, const double *pose,
                                    int64_t *stripOff_out, int64_t *memOff_out);

/* counts [5] of the resident tables: designs, strip records, member records, Kim & Yue rows, Kim & Yue items per heading */
int raftx_qtf_tables_counts(raftx_ctx *ctx, int64_t *counts);

/* The resident records on the host, for checking and for feeding raftx_qtf_slender: strips [nStrip,RAFTX_QS_N], members
 * [nMem,RAFTX_QM_N], kayOff [nDesign+1] (rows), kayNodes [nRow,RAFTX_QKG_N].  Any pointer may be NULL. */
int raftx_qtf_tables_fetch(raftx_ctx *ctx, double *strips, double *members, int64_t *kayOff, double *kayNodes);

/* The Kim & Yue items (RAFTX_QK_N doubles each, the records raftx_qtf_kay takes) the resident tables give for the headings
 * beta [nCase], set s = d * nCase + c: itemOff [nDesign*nCase+1], items [counts[4]*nCase,RAFTX_QK_N].  For checking. */
int raftx_qtf_tables_kay_items(raftx_ctx *ctx, int nCase, const double *beta, int64_t *itemOff, double *items);

/* raftx_qtf_slender on the resident tables: nDesign * nCase sets s = d * nCase + c, set s reads the table of design
 * s / nCase through an index (no copy per sea state) and the heading beta[c].  Xi [nSet,6,nw2] or NULL (the RAOs of the
 * resident first-order responses, as raftx_qtf_slender: their (design, case) pairs must be these sets).  Mstruc
 * [nDesign,6,6].  Nm > 0: the Kim & Yue correction of the MacCamy-Fuchs members with Nm + 1 terms, items and tables built
 * on the device; Nm == 0: none.  The result stays resident for raftx_qtf_force; qtf [nSet,nw2,nw2,6] may be NULL.
 * Launches the kernels of raftx_qtf_slender (and raftx_qtf_kay): the same bits as that entry fed the fetched records.
 * Device scratch per set, bytes: nw2 * (16 * (2 * 26 * S + 12 * M + 18) + ...) with S strips and M member records of its
 * design -- 832 nw2 S dominates (1.8 MB at S = 53, nw2 = 40) -- plus 96 nw2^2 for the result and as much again for the
 * Kim & Yue table.  A batch that does not fit fails with a message that states the bytes asked for; cutting it is the
 * caller's business.
 * Errors, all before any launch: no resident tables; nCase < 1; nw2 < 1; NULL w2 / k2 / beta / Mstruc; Nm outside
 * 0 .. 10; Xi == NULL without resident responses of nDesign * nCase pairs. */
int raftx_qtf_slender_resident(raftx_ctx *ctx, int nCase, int nw2, const double *w2, const double *k2, double depth,
                               double rho, double g, const raftx_c128 *Xi, const double *beta, const double *Mstruc,
                               int Nm, raftx_c128 *qtf);

#ifdef __cplusplus
}
#endif

#endif /* RAFTX_QTFGEN_H */
