// scipy's rectangular linear-sum-assignment for the set criteria (criterion.hip,
// criterion_sigma.hip): one lane, all state in LDS.
#pragma once
#include "spe_common.h"

namespace {

constexpr double LSAP_INF = 1.0e300;

// scipy's augmenting-path LSAP on an [nr][nc] row-major fp64 matrix in LDS (nr <= nc);
// col4row[r] = assigned column.  Sequential (one lane), in oracle/criterion_ref.lsap's order.
SPE_DEV void lsap_lane(const double* c, int nr, int nc, int* col4row, int* row4col, double* u, double* v,
                       double* spc, int* path, bool* sr, bool* sc, int* remaining) {
  for (int i = 0; i < nr; ++i) { u[i] = 0.0; col4row[i] = -1; }
  for (int j = 0; j < nc; ++j) { v[j] = 0.0; row4col[j] = -1; }
  for (int cur = 0; cur < nr; ++cur) {
    for (int j = 0; j < nc; ++j) { spc[j] = LSAP_INF; path[j] = -1; sc[j] = false; remaining[j] = nc - 1 - j; }
    for (int i = 0; i < nr; ++i) sr[i] = false;
    int nrem = nc, i = cur, sink = -1;
    double min_val = 0.0;
    while (sink == -1) {
      sr[i] = true;
      int index = -1;
      double lowest = LSAP_INF;
      for (int it = 0; it < nrem; ++it) {
        const int j = remaining[it];
        const double r = min_val + c[i * nc + j] - u[i] - v[j];
        if (r < spc[j]) { path[j] = i; spc[j] = r; }
        if (spc[j] < lowest || (spc[j] == lowest && row4col[j] == -1)) { lowest = spc[j]; index = it; }
      }
      min_val = lowest;
      if (index < 0 || !(min_val < LSAP_INF)) return;     // infeasible (non-finite costs): leave -1s
      const int j = remaining[index];
      if (row4col[j] == -1) sink = j;
      else i = row4col[j];
      sc[j] = true;
      remaining[index] = remaining[--nrem];
    }
    u[cur] += min_val;
    for (int r = 0; r < nr; ++r)
      if (sr[r] && r != cur) u[r] += min_val - spc[col4row[r]];
    for (int j = 0; j < nc; ++j)
      if (sc[j]) v[j] -= min_val - spc[j];
    int j = sink;
    while (true) {
      const int r = path[j];
      row4col[j] = r;
      const int t = col4row[r];
      col4row[r] = j;
      j = t;
      if (r == cur) break;
    }
  }
}

}  // namespace
