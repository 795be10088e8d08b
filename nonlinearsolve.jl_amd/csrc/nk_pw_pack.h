// The resident matrix-powers kernel's per-pattern operand table (nk_powers.hip) — plain C++, no HIP: what a workgroup needs
// to put its band of the matrix into registers, worked out ONCE per pattern on the host instead of once per launch on the
// device. The kernel used to re-read `rowptr` and `col` (4·(n + 1) + 4·nnz bytes) in every launch and to turn them, row by row,
// into the same numbers every time: the row's length, where its entries start inside its slice of `val`, and the ≤ W offsets of
// its columns in the band's LDS window [halo above | own rows | halo below]. None of it depends on the values.
//
// One RECORD per row, 16-bit fields (half-words h[0] … of NW 32-bit words):
//   h[0]          the row's first entry relative to its slice's first entry (k0 − kb); for odd W the row length sits in the
//                 bits above PW_START_BITS_ODD (W = 5: 13 + 3 bits — the record is 12 bytes),
//   h[1 + j]      j < W: the LDS offset of the j-th entry's column, c − (first row of the band − PW_HALO), a halo slot's column
//                 already replaced by its row next door; slots past the row's end hold the row's OWN offset (never summed),
//   h[W + 1]      even W: the row length (the spare half-word of the last word).
// W = 5: 3 words (12 bytes), W = 8: 5 words, W = 16: 9 words per row. Rows past the matrix' end are empty rows.
// Layout [band][slice][word][PW_T]: thread t of band b reads word k of its row of slice i at ((b·RPT + i)·NW + k)·PW_T + t —
// a wavefront's loads are lane-contiguous dwords. Beside it one {kb, ke} pair per (band, slice): the slice's extent in `val`.
//
// pw_pack REJECTS what does not fit (a row longer than W, a column outside the band's window, a halo slot without a row, a
// slice with more than PW_T·W entries): the caller then makes no plan and the matrix keeps the streaming kernel.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__HIPCC__)
#define PW_HD __host__ __device__
#else
#define PW_HD
#endif

constexpr int PW_T = 1024;      // threads per workgroup = rows per slice
constexpr int PW_HALO = 1024;   // rows a band may read from either neighbour
constexpr int PW_START_BITS_ODD = 13;

// field layout of a record for rows of ≤ W entries
template <int W>
struct pw_rec {
  static constexpr bool LEN_IN_H0 = (W % 2) == 1;                 // odd W: W + 1 half-words fill the words exactly
  static constexpr int NH = W + 1 + (LEN_IN_H0 ? 0 : 1);
  static constexpr int NW = NH / 2;
  static constexpr uint32_t START_MAX = LEN_IN_H0 ? (1u << PW_START_BITS_ODD) - 1 : 0xFFFFu;
  static constexpr uint32_t LEN_MAX = LEN_IN_H0 ? (1u << (16 - PW_START_BITS_ODD)) - 1 : 0xFFFFu;
  static constexpr uint32_t OFF_MAX = 0xFFFFu;
  static_assert(NH % 2 == 0, "whole words");
  static_assert(START_MAX >= (uint32_t)PW_T * W, "the row-start field holds every position of a staged slice");
  static_assert(LEN_MAX >= (uint32_t)W, "the length field holds W");
  // (w: the record's words, in registers on the device)
  PW_HD static uint32_t half(const uint32_t *w, int h) { return (w[h >> 1] >> ((h & 1) * 16)) & 0xFFFFu; }
  PW_HD static int start(const uint32_t *w) { return (int)(half(w, 0) & START_MAX); }
  PW_HD static int len(const uint32_t *w) { return LEN_IN_H0 ? (int)(half(w, 0) >> PW_START_BITS_ODD) : (int)half(w, W + 1); }
  PW_HD static int off(const uint32_t *w, int j) { return (int)half(w, 1 + j); }
};
// the same numbers for a run-time W (5, 8, 16)
inline int pw_rec_words(int w) { return (w + 1 + ((w % 2) ? 0 : 1)) / 2; }

struct pw_pack_in {
  int64_t n = 0;                     // rows
  const int32_t *rowptr = nullptr;   // [n + 1]
  const int32_t *col = nullptr;      // local columns: [0, n) owned, n + h = halo slot h
  int rpt = 0, w = 0, nb = 0;        // the layout pw_find_layout chose: slices per band, slots per row, bands
  const int32_t *hvl = nullptr;      // several ranks: halo slot → row relative to this rank's first row (negative: above); [nh]
  int nh = 0;
};
struct pw_pack_out {
  std::vector<uint32_t> rec;   // [nb][rpt][NW][PW_T]
  std::vector<int32_t> ext;    // [nb][rpt][2]: {kb, ke}
};
enum { PW_PACK_OK = 0, PW_PACK_E_ARG = 1, PW_PACK_E_LEN = 2, PW_PACK_E_RANGE = 3, PW_PACK_E_HALO = 4, PW_PACK_E_EXTENT = 5 };

inline int pw_pack(const pw_pack_in &in, pw_pack_out *out) {
  const int w = in.w, rpt = in.rpt;
  if (!out || !in.rowptr || !in.col || in.n < 1 || rpt < 1 || (w != 5 && w != 8 && w != 16) || in.nh < 0) return PW_PACK_E_ARG;
  const int64_t rb = (int64_t)PW_T * rpt, xn = rb + 2 * PW_HALO;
  if (xn - 1 > 0xFFFF || in.nb < 1 || (int64_t)in.nb != (in.n + rb - 1) / rb) return PW_PACK_E_ARG;
  const bool len_in_h0 = (w % 2) == 1;
  const uint32_t start_max = len_in_h0 ? (1u << PW_START_BITS_ODD) - 1 : 0xFFFFu;
  const int nw = pw_rec_words(w);
  out->rec.assign((size_t)in.nb * rpt * nw * PW_T, 0u);
  out->ext.assign((size_t)in.nb * rpt * 2, 0);
  for (int b = 0; b < in.nb; ++b)
    for (int i = 0; i < rpt; ++i) {
      const int64_t r0 = (int64_t)b * rb, rfirst = r0 + (int64_t)PW_T * i;
      const bool any = rfirst < in.n;
      const int64_t rl = any ? (rfirst + PW_T <= in.n ? rfirst + PW_T : in.n) : rfirst;
      const int32_t kb = any ? in.rowptr[rfirst] : 0, ke = any ? in.rowptr[rl] : 0;
      if (kb < 0 || ke < kb || (int64_t)ke - kb > (int64_t)PW_T * w) return PW_PACK_E_EXTENT;
      out->ext[((size_t)b * rpt + i) * 2] = kb;
      out->ext[((size_t)b * rpt + i) * 2 + 1] = ke;
      uint32_t *slice = out->rec.data() + ((size_t)b * rpt + i) * nw * PW_T;
      for (int t = 0; t < PW_T; ++t) {
        const int64_t r = rfirst + t;
        const uint32_t own = (uint32_t)(PW_HALO + t + PW_T * i);
        uint32_t h[18] = {};
        int len = 0;
        uint32_t start = 0;
        if (r < in.n) {
          const int32_t k0 = in.rowptr[r], k1 = in.rowptr[r + 1];
          if (k1 < k0 || k1 - k0 > w) return PW_PACK_E_LEN;
          if (k0 < kb || k1 > ke || (uint32_t)(k0 - kb) > start_max) return PW_PACK_E_EXTENT;
          len = k1 - k0;
          start = (uint32_t)(k0 - kb);
          for (int j = 0; j < len; ++j) {
            int64_t c = in.col[k0 + j];
            if (c < 0) return PW_PACK_E_RANGE;
            if (c >= in.n) {   // a halo slot → its row next door
              if (!in.hvl || c - in.n >= in.nh) return PW_PACK_E_HALO;
              c = in.hvl[c - in.n];
            }
            const int64_t o = c - (r0 - PW_HALO);
            if (o < 0 || o >= xn) return PW_PACK_E_RANGE;
            h[1 + j] = (uint32_t)o;
          }
        }
        for (int j = len; j < w; ++j) h[1 + j] = own;
        if (len_in_h0) h[0] = start | ((uint32_t)len << PW_START_BITS_ODD);
        else { h[0] = start; h[w + 1] = (uint32_t)len; }
        for (int k = 0; k < nw; ++k) slice[(size_t)k * PW_T + t] = h[2 * k] | (h[2 * k + 1] << 16);
      }
    }
  return PW_PACK_OK;
}
