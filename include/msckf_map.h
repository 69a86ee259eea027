/*
 * msckf_map.h -- the filter's feature map kept on the device: the bookkeeping
 * of a frame that msckf_hip.h leaves to the host (MSCKF.map_server, the dict of
 * Feature objects with their observation dicts) as tables of the msckf_ctx_t,
 * and the feature batch of an update gathered from them on the device (same
 * library, conventions of msckf_hip.h; errors through msckf_last_error()).
 *
 *   msckf_map_create         the filters' tables, in the context
 *   msckf_map_put / _get     whole-table write and read of one filter (tests,
 *                            inspection, a lane joining mid-stream)
 *   msckf_map_clear          empty tables (online reset)
 *   msckf_map_add_lost       add_feature_observations (msckf.py:409-427) and the
 *                            selection of remove_lost_features (616-660)
 *   msckf_map_prune_select   the selection of prune_cam_state_buffer (730-775)
 *   msckf_map_load           msckf_batch_load with the observations taken from
 *                            the tables
 *   msckf_map_prune_commit   the map side of msckf.py:776-818
 *
 * This text is the specification; tests/feature_map_ref.py restates it in numpy.
 *
 * ---------------------------------------------------------------------------
 * The table
 *
 * Each filter slot has cap rows (msckf_map_create; 1 <= cap <= 2048; a context
 * holds one set of tables, a second create is an error; msckf_destroy frees
 * them).  The first n rows are in use, in MAP ORDER: the insertion order of the
 * reference's map_server dict, where a deletion keeps the order of the rest.  A
 * row is
 *   id              int64
 *   mask            uint64[2]: bit s of word s / 64 = the feature has an
 *                   observation from cam slot s (n_cam_capacity <= 128)
 *   z[slot][4]      double, u0 v0 u1 v1 exactly as the message carried them;
 *                   defined only where the mask bit is set
 *   p_w[3]          double, and is_initialized uint8
 * A feature's observations are read in ascending cam slot: slots are oldest
 * first, so that is the insertion order of the reference's observation dict.
 *
 * There are two tables per slot.  A call that changes a table reads the current
 * one and writes the other; the library makes the written one current only
 * after the call succeeded, so an error leaves every current table as it was
 * (the lost table of msckf_map_add_lost, below, does not outlive a failed call
 * that wrote over it).  The row
 * count n and which table is current are the host library's record; the device
 * reads them from the call's header.  chi2_table: the 99 thresholds of
 * chi_squared_test_table (dof 1..99), uploaded once.
 *
 * msckf_map_put writes n rows (ids distinct, no mask bit at or beyond
 * n_cam_capacity; z is [n][n_cam_capacity][4]) -- n > cap is -3.  msckf_map_get
 * returns the current table (arrays sized for cap rows; z entries without a
 * mask bit are returned as 0).  msckf_map_clear sets n = 0.
 *
 * Every call below takes nfilt distinct filter slots and serves all of them in
 * one launch per stage; arguments of every filter are checked on the host
 * before anything is copied or launched (-1).  Each packs its inputs into one
 * block and makes one host-to-device copy.
 *
 * ---------------------------------------------------------------------------
 * msckf_map_add_lost
 *
 * Per filter w the message is rows [msg_off[w], msg_off[w+1]) of ids / z
 * (double [.][4]).  Ids within one message must be distinct (-1, found on the
 * host before anything is copied).  s = the filter's newest cam slot (n_cams -
 * 1; a filter without cam states is -1).  Per filter:
 *  1. Every message row is matched against the table's ids.  tracked = the
 *     matched rows; n_before = n.
 *  2. The unmatched rows are appended in message order: id, empty mask, p_w =
 *     0, is_initialized = 0.  More than cap rows: the call returns -3 and no
 *     table of any named filter changes.
 *  3. Every matched or appended row gets mask bit s and z[s] = the message's.
 *  4. Every row without bit s is classified by its observation count M (the
 *     set bits): M < 3 invalid, otherwise a candidate.
 *  5. Both kinds are removed: the next table is the remaining rows in order.
 *  6. The descriptor lists the candidates in map order: id, and info[4] = (M,
 *     0, is_initialized, row) with row the candidate's row in the table the
 *     call READ.  That table stays intact as the filter's "lost table" until
 *     the filter's next put, add_lost, prune_select or prune_commit -- a failed
 *     add_lost or prune_select included: the launch has written the set the
 *     lost table lived in, and a lost-form load is then refused (-1) until the
 *     next good add_lost.  The lost form of msckf_map_load reads the
 *     candidates from it.
 * The host forms tracking_rate = tracked / (n_before + 1e-5).  One
 * device-to-host copy and one synchronisation return the counts and the
 * descriptors.
 *
 * ---------------------------------------------------------------------------
 * msckf_map_prune_select
 *
 * Per filter the cam slots to remove, cam_slots[slot_off[w] .. slot_off[w+1])
 * (distinct, below n_cams).  For every row, k = its observations from those
 * slots: k = 1: the observation is dropped (mask bit cleared); k >= 2: the row
 * is INVOLVED and keeps everything.  No row moves.  The descriptor lists the
 * involved rows in map order: id, and info[4] = (M, k, is_initialized, row),
 * M the row's whole observation count.  The removed slots stay recorded with
 * the filter (the select is "open") until msckf_map_prune_commit.  One copy
 * back and one synchronisation, as above.
 *
 * ---------------------------------------------------------------------------
 * msckf_map_load
 *
 * What msckf_batch_load does, with the loader's fill (obs_cam, obs_z, p_w,
 * valid, chi2) gathered from the tables instead of copied from the host.  The
 * features of filter w are rows[feat_off[w] .. feat_off[w+1]) with counts[.]
 * observations each, both as the descriptors gave them.  The host can check
 * rows and counts only for their ranges; a count that is not the descriptor's
 * stays inside every buffer but gives an undefined batch (a count above the
 * row's observations is padded with cam slot 0, which the update chain does
 * not accept twice in a feature).  The batch holds the features in ascending
 * filter slot, each filter's in the order given; unnamed filters get none.
 * Observations are listed in ascending cam slot and
 * cast to the context's scalar as the host loader casts them.  Forms:
 *   MSCKF_MAP_LOAD_LOST          rows of the lost table, all observations;
 *       chi2 = table[M - 1 dof]; p_w = the row's if is_initialized (valid = 2),
 *       NaN otherwise (valid = 0: triangulated inside msckf_batch_update).
 *   MSCKF_MAP_LOAD_PRUNE_TRI     rows of the current table (after the open
 *       select), all observations; no chi2 (as msckf_batch_load without one),
 *       valid = 0: for msckf_batch_triangulate.
 *   MSCKF_MAP_LOAD_PRUNE_UPDATE  rows of the current table, only the
 *       observations from the removed slots (counts = k); chi2 = table[k dof];
 *       p_w = the caller's row of p_w where it is finite (a position
 *       msckf_batch_triangulate just returned), the table's otherwise; p_w may
 *       be NULL.
 * A dof outside 1..99 is -1 before anything changes (the host path raises
 * KeyError), as is a form that does not follow its select call.  The loaded
 * batch is run by msckf_batch_triangulate / msckf_batch_update and read by
 * msckf_batch_results / msckf_readback, unchanged.  Asynchronous.
 *
 * ---------------------------------------------------------------------------
 * msckf_map_prune_commit
 *
 * Closes the open select of each named filter.  Entries rows / valid / p_w
 * [ent_off[w] .. ent_off[w+1]) are the rows msckf_batch_triangulate was run
 * for (distinct): p_w and is_initialized = valid are stored in them, whether
 * the triangulation succeeded or not (feature.py sets both).  Then, in every
 * row, the observations from the removed slots are dropped -- the involved
 * observations of the rows that took part in the update and of the rows whose
 * triangulation failed; no other is left after the select -- and mask and z
 * move to the cam slots that remain: an observation of slot s goes to s minus
 * the removed slots below s, which is the slot msckf_prune_batch gives that
 * cam.  Asynchronous; no row moves.
 *
 * Kernels (csrc/msckf_map.hip): one workgroup of four wavefronts per named
 * filter; fixed-stride [filter][cap] tables; the id match against the table's
 * ids staged in LDS (cap 8 B); order-preserving compactions by ballot rank,
 * the wave counts through LDS in wave order; no atomics, no data-dependent
 * order: a repeat gives the same bits.
 */
#ifndef MSCKF_MAP_H
#define MSCKF_MAP_H

#include <stdint.h>

#include "msckf_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#define MSCKF_MAP_LOAD_LOST 0
#define MSCKF_MAP_LOAD_PRUNE_TRI 1
#define MSCKF_MAP_LOAD_PRUNE_UPDATE 2
#define MSCKF_MAP_INFO 4      /* int32 per descriptor entry */
#define MSCKF_MAP_CHI2_LEN 99 /* dof 1..99 */

int msckf_map_create(msckf_ctx_t* ctx, int cap, const double* chi2_table);
int msckf_map_clear(msckf_ctx_t* ctx, int nfilt, const int32_t* filters);

/* ids int64 [n], mask uint64 [n][2], z double [n][n_cam_capacity][4], p_w double [n][3], initialized uint8 [n] */
int msckf_map_put(msckf_ctx_t* ctx, int filter, int n, const int64_t* ids, const uint64_t* mask, const double* z,
                  const double* p_w, const uint8_t* initialized);
/* outputs sized for cap rows (any may be NULL but n_out); *n_out rows are written */
int msckf_map_get(msckf_ctx_t* ctx, int filter, int32_t* n_out, int64_t* ids, uint64_t* mask, double* z, double* p_w,
                  uint8_t* initialized);

/* Outputs: tracked, n_before, n_cand int32 [nfilt]; desc_id int64 [nfilt][cap], desc_info int32
 * [nfilt][cap][MSCKF_MAP_INFO] (the first n_cand entries of each filter). */
int msckf_map_add_lost(msckf_ctx_t* ctx, int nfilt, const int32_t* filters, const int32_t* msg_off, const int64_t* ids,
                       const double* z, int32_t* tracked_out, int32_t* n_before_out, int32_t* n_cand_out,
                       int64_t* desc_id_out, int32_t* desc_info_out);

/* Outputs: n_inv int32 [nfilt]; the descriptors as above (the first n_inv entries of each filter). */
int msckf_map_prune_select(msckf_ctx_t* ctx, int nfilt, const int32_t* filters, const int32_t* slot_off,
                           const int32_t* cam_slots, int32_t* n_inv_out, int64_t* desc_id_out,
                           int32_t* desc_info_out);

/* rows, counts int32 [feat_off[nfilt]]; p_w double [feat_off[nfilt]][3] or NULL */
int msckf_map_load(msckf_ctx_t* ctx, int mode, int nfilt, const int32_t* filters, const int32_t* feat_off,
                   const int32_t* rows, const int32_t* counts, const double* p_w);

/* rows int32, valid uint8, p_w double [.][3], ent_off[nfilt] entries */
int msckf_map_prune_commit(msckf_ctx_t* ctx, int nfilt, const int32_t* filters, const int32_t* ent_off,
                           const int32_t* rows, const uint8_t* valid, const double* p_w);

#ifdef __cplusplus
}
#endif
#endif /* MSCKF_MAP_H */
