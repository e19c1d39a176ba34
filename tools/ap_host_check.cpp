// The two index rules of csrc/ap.cuh as a stand-alone host program, for the host sanitizers (no GPU, nothing loaded into Python):
//
//   hipcc --offload-arch=gfx950 -std=c++17 -ffp-contract=off -Xarch_host -fsanitize=address,undefined \
//         -Xarch_host -fno-sanitize-recover=undefined tools/ap_host_check.cpp -o ap_host_check && ./ap_host_check
//
// 1. the radix ranking: a tile's rows go through ap_same_digit / ap_rank_below / ap_tile_rank round by round and wave by wave, as
//    k_ap_scatter takes them (the ballots are formed here lane by lane), and must land where a stable counting sort puts them -- at row
//    counts around a wave and the tile, with digits drawn from 1, 2, 3 and 256 values;
// 2. np.interp's index rule: ap_interp_pr / ap_interp_conf over a host view of one class against a plain linear-search statement of the rule,
//    on abscissae with long runs of repeats (recall reaching 1.0 early, equal confidences), at every grid point and at the abscissae themselves.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../mga_yolo_amd/csrc/ap.cuh"

using namespace mgacbam;

static unsigned g_seed = 12345u;
static unsigned rnd() { g_seed = g_seed * 1664525u + 1013904223u; return g_seed >> 8; }

static int check_ranking(int n, unsigned values) {
  std::vector<unsigned> digit(n);
  for (int i = 0; i < n; ++i) digit[i] = rnd() % values;
  std::vector<int> first(257, 0), want(n), got(n, -1);
  for (int i = 0; i < n; ++i) ++first[digit[i] + 1];
  for (int d = 0; d < 256; ++d) first[d + 1] += first[d];
  std::vector<int> next(first.begin(), first.end() - 1);
  for (int i = 0; i < n; ++i) want[i] = next[digit[i]]++;
  std::vector<int> run(256, 0);
  static int cnt[kApWaves][256];
  for (int r = 0; r < kApPer; ++r) {
    for (int w = 0; w < kApWaves; ++w) for (int d = 0; d < 256; ++d) cnt[w][d] = 0;
    unsigned long long same[kApWaves][kWave];
    for (int w = 0; w < kApWaves; ++w) {
      const int p0 = (r * kApWaves + w) * kWave;
      unsigned long long live = 0, have[8] = {0};
      for (int l = 0; l < kWave; ++l) {
        if (p0 + l >= n) continue;
        live |= 1ull << l;
        for (int b = 0; b < 8; ++b) if ((digit[p0 + l] >> b) & 1u) have[b] |= 1ull << l;
      }
      for (int l = 0; l < kWave; ++l) {
        const unsigned d = p0 + l < n ? digit[p0 + l] : 0u;
        same[w][l] = ap_same_digit(live, have, d);
        if (p0 + l < n && ap_rank_below(same[w][l], l) == 0) cnt[w][d] = __builtin_popcountll(same[w][l]);
      }
    }
    for (int w = 0; w < kApWaves; ++w)
      for (int l = 0; l < kWave; ++l) {
        const int p = (r * kApWaves + w) * kWave + l;
        if (p < n) got[p] = first[digit[p]] + ap_tile_rank(run[digit[p]], cnt, w, digit[p], ap_rank_below(same[w][l], l));
      }
    for (int d = 0; d < 256; ++d) for (int w = 0; w < kApWaves; ++w) run[d] += cnt[w][d];
  }
  for (int i = 0; i < n; ++i)
    if (got[i] != want[i]) { std::printf("ranking: n=%d values=%u row %d lands at %d, a stable sort puts it at %d\n", n, values, i, got[i], want[i]); return 1; }
  return 0;
}

struct HostView {                                              // one class, as ApClass shows it
  std::vector<int> tpc; std::vector<double> env, conf; int np_; double den;
  double recall(int j) const { return static_cast<double>(tpc.at(j)) / den; }
  double precision(int j) const { return static_cast<double>(tpc.at(j)) / static_cast<double>(j + 1); }
  double mrec(int j) const { return j == 0 ? 0.0 : (j == np_ + 1 ? 1.0 : recall(j - 1)); }
  double mpre(int j) const { return j == 0 ? 1.0 : (j == np_ + 1 ? 0.0 : env.at(j - 1)); }
  double neg_conf(int j) const { return -conf.at(j); }
};
// the rule by a linear search from the right: the LAST j with xp[j] <= x
template <typename XP, typename FP>
static double interp_linear(int len, XP xp, FP fp, double x, double left) {
  if (x < xp(0)) return left;
  int j = len - 1;
  while (xp(j) > x) --j;
  if (j == len - 1 || xp(j) == x) return fp(j);
  return (fp(j + 1) - fp(j)) / (xp(j + 1) - xp(j)) * (x - xp(j)) + fp(j);
}

static int check_interp(int np_, int nt, int distinct_conf) {
  HostView K;
  K.np_ = np_; K.den = static_cast<double>(nt) + 1e-16;
  int tp = 0;
  double c = 1.0;
  for (int j = 0; j < np_; ++j) {
    if (tp < nt && rnd() % 3 == 0) ++tp;
    K.tpc.push_back(tp);
    if (j == 0 || rnd() % distinct_conf != 0) c -= 1.0 / (np_ + 2);          // distinct_conf = 1: every confidence repeats the first
    K.conf.push_back(c);
  }
  K.env.assign(np_, 0.0);
  double m = 0.0;
  for (int j = np_ - 1; j >= 0; --j) { m = K.precision(j) > m ? K.precision(j) : m; K.env[j] = m; }
  std::vector<double> xs;
  for (int k = 0; k < 1000; ++k) xs.push_back(k / 999.0);
  for (int j = 0; j <= np_ + 1; ++j) xs.push_back(K.mrec(j));
  for (int j = 0; j < np_; ++j) if (K.conf[j] >= 0) xs.push_back(K.conf[j]);
  for (double x : xs) {
    const double a = ap_interp_pr(K, x), b = interp_linear(np_ + 2, [&](int j) { return K.mrec(j); }, [&](int j) { return K.mpre(j); }, x, 1.0);
    const double r = ap_interp_conf<true>(K, x, 0.0), r2 = interp_linear(np_, [&](int j) { return K.neg_conf(j); }, [&](int j) { return K.recall(j); }, -x, 0.0);
    const double p = ap_interp_conf<false>(K, x, 1.0), p2 = interp_linear(np_, [&](int j) { return K.neg_conf(j); }, [&](int j) { return K.precision(j); }, -x, 1.0);
    if (a != b || r != r2 || p != p2) { std::printf("interp: np=%d nt=%d x=%.17g: %.17g %.17g | %.17g %.17g | %.17g %.17g\n", np_, nt, x, a, b, r, r2, p, p2); return 1; }
  }
  return 0;
}

int main() {
  int bad = 0, runs = 0;
  for (int n : {1, 63, 64, 65, 255, 256, 257, 2047, 2048})
    for (unsigned values : {1u, 2u, 3u, 256u}) { bad += check_ranking(n, values); ++runs; }
  for (int np_ : {1, 2, 3, 7, 64, 1000})
    for (int nt : {1, 2, 5, 400})
      for (int distinct : {1, 2, 1000}) { bad += check_interp(np_, nt, distinct); ++runs; }
  std::printf("%d checks, %d failed\n", runs, bad);
  return bad ? 1 : 0;
}
