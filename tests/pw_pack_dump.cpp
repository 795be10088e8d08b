// Test driver of csrc/nk_pw_pack.h (tests/test_pw_pack.py): reads a CSR pattern and a band layout from a file of int32 words,
// packs the resident matrix-powers kernel's operand table and writes it back DECODED — through the accessors the kernel itself
// uses (pw_rec<W>) — as int32 words on stdout:
//   in : n, nnz, rpt, w, nb, nh, rowptr[n + 1], col[nnz], hvl[nh]
//   out: status; on PW_PACK_OK for every row of every band (nb · rpt · PW_T rows, in row order): len, start, off[0 … w − 1];
//        then kb, ke for every (band, slice)
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "nk_pw_pack.h"

template <int W>
static void decode(const pw_pack_out &T, int nb, int rpt, std::vector<int32_t> &out) {
  constexpr int NW = pw_rec<W>::NW;
  for (int b = 0; b < nb; ++b)
    for (int i = 0; i < rpt; ++i)
      for (int t = 0; t < PW_T; ++t) {
        uint32_t w[NW];
        for (int k = 0; k < NW; ++k) w[k] = T.rec[(((size_t)b * rpt + i) * NW + k) * PW_T + t];
        out.push_back(pw_rec<W>::len(w));
        out.push_back(pw_rec<W>::start(w));
        for (int j = 0; j < W; ++j) out.push_back(pw_rec<W>::off(w, j));
      }
}

int main(int argc, char **argv) {
  if (argc != 2) return 2;
  FILE *f = fopen(argv[1], "rb");
  if (!f) return 2;
  int32_t hd[6];
  if (fread(hd, sizeof(int32_t), 6, f) != 6) return 2;
  const int n = hd[0], nnz = hd[1], rpt = hd[2], w = hd[3], nb = hd[4], nh = hd[5];
  if (n < 0 || nnz < 0 || nh < 0) return 2;
  std::vector<int32_t> rowptr((size_t)n + 1), col((size_t)nnz), hvl((size_t)nh);
  if (fread(rowptr.data(), sizeof(int32_t), rowptr.size(), f) != rowptr.size()) return 2;
  if (nnz && fread(col.data(), sizeof(int32_t), col.size(), f) != col.size()) return 2;
  if (nh && fread(hvl.data(), sizeof(int32_t), hvl.size(), f) != hvl.size()) return 2;
  fclose(f);
  pw_pack_in in;
  in.n = n; in.rowptr = rowptr.data(); in.col = col.data(); in.rpt = rpt; in.w = w; in.nb = nb;
  in.hvl = nh ? hvl.data() : nullptr; in.nh = nh;
  pw_pack_out T;
  const int rc = pw_pack(in, &T);
  std::vector<int32_t> out;
  out.push_back(rc);
  if (rc == PW_PACK_OK) {
    if ((int)T.rec.size() != nb * rpt * pw_rec_words(w) * PW_T || (int)T.ext.size() != nb * rpt * 2) return 3;
    if (w == 5) decode<5>(T, nb, rpt, out);
    else if (w == 8) decode<8>(T, nb, rpt, out);
    else decode<16>(T, nb, rpt, out);
    out.insert(out.end(), T.ext.begin(), T.ext.end());
  }
  return fwrite(out.data(), sizeof(int32_t), out.size(), stdout) == out.size() ? 0 : 4;
}
