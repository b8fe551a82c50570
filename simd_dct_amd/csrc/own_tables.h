// own_tables.h -- the multiplier tables of the engine-own paths (OwnTables, mdct_kernels.h), derived on the host.  Shared by
// mdct_api.hip (libmdct_hip.so) and the scan coders (scan_host.h: libmdct_jpegenc_scan.so, libmdct_jpegenc_opt.so): one derivation, so
// the same coefficients.
#pragma once
#include <cmath>
#include <cstring>
#include <mutex>

#include "mdct_kernels.h"

namespace mdct
{

// AAN scale factors a_0 = 1, a_k = sqrt(2) cos(k pi / 16); the 2-D tables are products of
// doubles rounded once to float (the CPU checker uses the identical expression).
constexpr double kAanScale[8] = {1.0, 1.387039845322148, 1.306562964876377, 1.175875602419359, 1.0, 0.785694958387102, 0.541196100146197, 0.275899379282943};

inline void aan_tables_compute(float *fwd, float *inv)
{
  for (int v = 0; v < 8; v++)
    for (int u = 0; u < 8; u++)
    {
      const double a = kAanScale[v] * kAanScale[u];
      fwd[v * 8 + u] = (float)(1.0 / (8.0 * a));
      inv[v * 8 + u] = (float)(a / 8.0);
    }
}

inline void aan_tables(float *fwd, float *inv)
{
  static float s_fwd[64], s_inv[64];
  static std::once_flag once;
  std::call_once(once, [] { aan_tables_compute(s_fwd, s_inv); });
  memcpy(fwd, s_fwd, sizeof(s_fwd));
  memcpy(inv, s_inv, sizeof(s_inv));
}

// forward multiplier = (1/lut) * scale, inverse multiplier = lut * scale, each one float op
// pair_order: the packed-fp32 kernels want both tables in the register-pair order of their column pass, j-major:
// (j*8 + v)*2 + {0,1} = (v, A[j]) / (v, B[j]) with A = {0,2,5,1}, B = {4,6,3,7}, the pairs aan_fwd_h produces (aan_fwd.h)
// Returns -1, or the index of the first entry of lut that is not finite and non-zero (tb is then not complete).
inline int own_tables_fill(const float *lut, OwnTables &tb, bool pair_order)
{
  float ft[64], it[64];
  aan_tables(ft, it);
  for (int i = 0; i < 64; i++)
  {
    if (lut && !(std::isfinite(lut[i]) && lut[i] != 0.0f))
      return i;
    tb.qf[i] = lut ? (1.0f / lut[i]) * ft[i] : ft[i];
    tb.dq[i] = lut ? lut[i] * it[i] : it[i];
  }
  if (pair_order)
  {
    static const int pa[4] = {0, 2, 5, 1}, pb[4] = {4, 6, 3, 7};
    OwnTables t = tb;
    for (int v = 0; v < 8; v++)
      for (int j = 0; j < 4; j++)
      {
        tb.qf[(j * 8 + v) * 2] = t.qf[v * 8 + pa[j]];
        tb.qf[(j * 8 + v) * 2 + 1] = t.qf[v * 8 + pb[j]];
        tb.dq[(j * 8 + v) * 2] = t.dq[v * 8 + pa[j]];
        tb.dq[(j * 8 + v) * 2 + 1] = t.dq[v * 8 + pb[j]];
      }
  }
  return -1;
}

} // namespace mdct
