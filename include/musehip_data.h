/* musehip_data.h - the dataset loader's entry points of libmusehip.so / libmusehip_dbg.so (csrc/loader.hip).
 *
 * A second header beside musehip.h: the training-data side of the library (MuseDiffusion/data/__init__.py load_data_music and what
 * stands behind it) lives here under the prefix mhd_, so that musehip.h stays the ABI of the model side.  Everything else is shared:
 * mh_stream_t, the mh_status return codes, and the error text, which is read through mh_last_error().
 *
 * Conventions as in musehip.h "batch producers": sequences are ragged, `values` = all rows back to back (int32), `offsets[B + 1]`
 * int64 row starts; one 256-thread block per row; int32 tokens throughout.  Any token value, index and draw is legal input: a row
 * that cannot be served gets a status, and nothing is read or written outside the buffers. */
#ifndef MUSEHIP_DATA_H
#define MUSEHIP_DATA_H

#include "musehip.h"

#ifdef __cplusplus
extern "C" {
#endif

enum mhd_gather_status {
  MHD_GATHER_OK = 0,
  MHD_GATHER_BAD_INDEX = 1, /* idx[b] outside [0, n): the row is empty */
  MHD_GATHER_OVERFLOW = 2   /* the rows up to and including this one do not fit cap: the row is empty */
};

enum mhd_augment_status {
  MHD_AUGMENT_OK = 0,
  MHD_AUGMENT_NOT_ORIGIN = 1,  /* the key token (index 1) is neither 602 (cmajor) nor 623 (aminor): commu/preprocessor/preprocessor.py:231-234 */
  MHD_AUGMENT_PITCH_RANGE = 2, /* some pitch would leave 0..127: augment_by_key's dump raises and the file is dropped (augment.py:64-69) */
  MHD_AUGMENT_BAD_ROW = 3      /* fewer than 12 tokens, more than mh_batch_max_row(), or a draw outside key -6..5 / tempo -2..2 */
};

/* Ragged gather, first launch: row b of the output is row idx[b] of a ragged source with n rows (src_offsets[n + 1]).
 * length[b] = its length, out_offsets[B + 1] = the exclusive scan of the lengths (one block loops over B; B <= 65536),
 * status[b] an mhd_gather_status.  An index outside [0, n) gives length 0; so does every row whose end would pass cap
 * (out_offsets stops growing there), so a values buffer of cap tokens is never overrun. */
int mhd_gather_offsets(const int64_t* src_offsets, int64_t n, const int64_t* idx, int64_t* out_offsets, int32_t* length, int32_t* status,
                       int B, int64_t cap, mh_stream_t stream);
/* Ragged gather, one launch per field: out[out_offsets[b] + j] = src_values[src_offsets[idx[b]] + j], j < length[b].
 * out_offsets / length: what mhd_gather_offsets wrote for the same (src_offsets, n, idx, cap); fields that share the
 * source offsets share them. */
int mhd_gather_rows(const int32_t* src_values, const int64_t* src_offsets, int64_t n, const int64_t* idx, const int64_t* out_offsets,
                    const int32_t* length, int32_t* out, int B, int64_t cap, mh_stream_t stream);
/* Ragged row select: out row b = take_b[b] != 0 ? row b of b_values : row b of a_values; the three buffers share `offsets`.
 * out may be a_values (rows that keep a are then left alone). */
int mhd_select_rows(const int32_t* a_values, const int32_t* b_values, const int64_t* offsets, const int32_t* take_b, int32_t* out, int B,
                    mh_stream_t stream);
/* Key / tempo augmentation of merged model rows (commu/preprocessor/augment.py as a token map), k = key_change[b] in -6..5,
 * c = bpm_change[b] in -2..2:
 *   index 0        560 + m, 1 <= m <= 40         -> 560 + min(max(m + c, 1), 40)        (encode_bpm of bpm + 5 c)
 *   index 1        602 + i or 614 + i, i < 12    -> the same base + (i + k) mod 12       (augment_by_key's MAJOR_KEY / MINOR_KEY walk)
 *   index >= 11    pitch token p in 3..130       -> p + k
 *   index >= 11    chord 195 + 9 r + q, r < 12   -> 195 + 9 ((r + k) mod 12) + q         (sync_key_augment; 303 = Chord_NN stays)
 * and every other token is copied.  status[b] (may be NULL) an mhd_augment_status; a row whose status is not OK is copied
 * unchanged (the reference produces no variant of it).  out may be values. */
int mhd_augment_rows(const int32_t* values, const int64_t* offsets, const int32_t* key_change, const int32_t* bpm_change, int32_t* out,
                     int32_t* status, int B, mh_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* MUSEHIP_DATA_H */
