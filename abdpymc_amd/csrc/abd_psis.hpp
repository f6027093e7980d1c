// abd_psis.hpp -- Pareto-smoothed importance sampling leave-one-out over the columns of a resident log-likelihood matrix
// (DESIGN 27).  The core knows nothing of survival models: it takes (matrix, ld, capacity, S, n_cells).
//
// Storage: unit-major, mat[unit][capacity]; the S draws of a unit are the first S doubles of its row.  abd_psis_store moves
// the n <= 16 rows of a launch from a [points][ld] buffer into it, thread = unit, n consecutive doubles each.
//
// abd_psis_kernel<VPT>: one 256-thread workgroup per unit, S <= 256 VPT; thread t holds draws t, t + 256, ... in registers as
// order-preserving 64-bit keys of x = (-ll) - max(-ll).  Per unit, exactly the estimator of DESIGN 27:
//   1. max(-ll), max(ll), sum exp(ll - max ll)                                       -> lppd
//   2. the (M + 1)-th largest x by a bitwise radix select on the keys (64 counts, integers: exact) -> cut
//   3. the tail {x > cut} compacted into LDS by a block scan of the per-thread counts, padded with +inf to a power of two and
//      sorted by a bitonic network on (x, draw): the draw index makes ties, and so the result, independent of the compaction
//   4. Zhang & Stephens' fit: wave w takes the grid points j = w + 1, w + 5, ...; lane l sums log1p(-b_j t_i) over i = l, l + 64,
//      ... in ascending order, then the wave's butterfly; the weights and b in ascending j; k and sigma
//   5. the smoothed values go to LDS under the tail's compaction index, where the thread that holds the draw finds them
//   6. logsumexp(x'), then logsumexp(ll + (x' - that)) with ll read again (the row is in L2)  -> elpd_loo
// Every floating-point sum: the thread's terms in ascending draw index, the butterfly over the lanes (xor 32, 16, ... 1), the
// four waves in ascending order.  The order depends on S (and on n_tail, a function of the data) alone: the result is the same
// bits however the matrix was filled.  No atomics.  LDS: 14.6 KiB, static.
#pragma once

#include <cmath>
#include <cstdint>
#include <cstring>
#include <limits>

#include <hip/hip_runtime.h>

namespace abdi {

constexpr int kPsisThreads = 256;
constexpr int kPsisTail = 512;  // the tail buffer: M <= 384 at the cap of 16384 draws
constexpr int kPsisGrid = 64;   // grid points of the fit: 30 + floor(sqrt(n_tail)) <= 52
constexpr int kPsisMaxDraws = 16384;

// M of S draws: min(S / 5, ceil(3 sqrt(S)))
inline int psis_tail_len(int64_t S) {
  const int64_t a = S / 5, b = (int64_t)std::ceil(3.0 * std::sqrt((double)S));
  return (int)(a < b ? a : b);
}

struct PsisArgs {
  const double* mat;       // [ld][capacity]
  const int32_t* n_cells;  // [ld]: a unit with 0 is left out (elpd = lppd = 0, k = NaN, n_tail = 0)
  double* elpd;            // [ld]
  double* pareto_k;        // [ld]
  double* lppd;            // [ld]
  int32_t* n_tail;         // [ld]
  int64_t capacity;
  int32_t S, M;
  double log_S, log_tiny;  // log S, log DBL_MIN: the host's
};

// rows 0 .. n - 1 of ll [n][ld] to the draws n0 .. n0 + n - 1 of mat [ld][capacity] (static: the header is compiled into two
// translation units, and only abd_survival.hip launches this one)
static __global__ __launch_bounds__(256) void abd_psis_store(const double* ll, double* mat, int32_t ld, int64_t capacity, int32_t n, int64_t n0) {
  const int unit = blockIdx.x * 256 + threadIdx.x;
  if (unit >= ld) return;
  double* row = mat + (int64_t)unit * capacity + n0;
  for (int p = 0; p < n; ++p) row[p] = ll[(int64_t)p * ld + unit];
}

__device__ inline uint64_t psis_key(double x) {  // order-preserving: x < y <=> key(x) < key(y)
  const uint64_t b = (uint64_t)__double_as_longlong(x);
  return (b >> 63) ? ~b : (b | 0x8000000000000000ull);
}
__device__ inline double psis_unkey(uint64_t k) {
  return __longlong_as_double((long long)((k >> 63) ? (k & 0x7fffffffffffffffull) : ~k));
}

struct PsisSum {
  template <typename T>
  __device__ T operator()(T a, T b) const { return a + b; }
};
struct PsisMax {
  __device__ double operator()(double a, double b) const { return fmax(a, b); }
};

template <typename T, typename Op>
__device__ inline T psis_wave_reduce(T v, Op op) {
  for (int o = 32; o > 0; o >>= 1) v = op(v, __shfl_xor(v, o));
  return v;
}

// The block's reduction, the same bits in every thread.  red [2][4]: the calls alternate between the halves, so that one barrier
// per call is enough (a thread writes a half again only after the barrier of the call in between, which every thread reaches after
// its reads of that half).
template <typename T, typename Op>
__device__ inline T psis_block_reduce(T v, Op op, T (*red)[4], int& phase) {
  v = psis_wave_reduce(v, op);
  if ((threadIdx.x & 63) == 0) red[phase][threadIdx.x >> 6] = v;
  __syncthreads();
  const T r = op(op(op(red[phase][0], red[phase][1]), red[phase][2]), red[phase][3]);
  phase ^= 1;
  return r;
}

template <int VPT>
__global__ __launch_bounds__(256) void abd_psis_kernel(const PsisArgs a) {
  __shared__ double tail_v[kPsisTail];    // the tail's x, sorted; then t_i = exp(x_(i)) - exp(cut)
  __shared__ uint32_t tail_p[kPsisTail];  // draw << 9 | compaction index
  __shared__ double smooth[kPsisTail];    // the smoothed value, by compaction index
  __shared__ double grid_b[kPsisGrid], grid_l[kPsisGrid], grid_w[kPsisGrid];
  __shared__ double red_d[2][4];
  __shared__ int red_i[2][4];
  __shared__ int wave_off[4];

  const int unit = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
  const int S = a.S;
  if (a.n_cells[unit] == 0) {  // the whole block
    if (tid == 0) {
      a.elpd[unit] = 0.0;
      a.lppd[unit] = 0.0;
      a.pareto_k[unit] = __longlong_as_double(0x7ff8000000000000ll);
      a.n_tail[unit] = 0;
    }
    return;
  }
  const double* row = a.mat + (int64_t)unit * a.capacity;
  int ph_d = 0, ph_i = 0;

  // 1. the row; lppd
  uint64_t key[VPT];
  double lppd;
  {
    double v[VPT];
    double mneg = -INFINITY, mpos = -INFINITY;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
      const int d = i * kPsisThreads + tid;
      v[i] = d < S ? row[d] : 0.0;
      if (d < S) {
        mneg = fmax(mneg, -v[i]);
        mpos = fmax(mpos, v[i]);
      }
    }
    mneg = psis_block_reduce(mneg, PsisMax(), red_d, ph_d);
    mpos = psis_block_reduce(mpos, PsisMax(), red_d, ph_d);
    double se = 0.0;
#pragma unroll
    for (int i = 0; i < VPT; ++i)
      if (i * kPsisThreads + tid < S) se += exp(v[i] - mpos);
    se = psis_block_reduce(se, PsisSum(), red_d, ph_d);
    lppd = (mpos + log(se)) - a.log_S;
#pragma unroll
    for (int i = 0; i < VPT; ++i) key[i] = psis_key(-v[i] - mneg);
  }

  // 2. the (M + 1)-th largest key
  uint64_t prefix = 0;
  int want = a.M + 1;
  for (int bit = 63; bit >= 0; --bit) {
    const uint64_t cand = (prefix | (1ull << bit)) >> bit;
    int c = 0;
#pragma unroll
    for (int i = 0; i < VPT; ++i) c += (i * kPsisThreads + tid < S && (key[i] >> bit) == cand) ? 1 : 0;
    c = psis_block_reduce(c, PsisSum(), red_i, ph_i);
    if (c >= want)
      prefix |= 1ull << bit;
    else
      want -= c;
  }
  const double cut = fmax(psis_unkey(prefix), a.log_tiny);
  const double ecut = exp(cut);

  // 3. the tail into LDS: the thread's first compaction index from a scan of the counts
  int mine = 0;
#pragma unroll
  for (int i = 0; i < VPT; ++i) mine += (i * kPsisThreads + tid < S && psis_unkey(key[i]) > cut) ? 1 : 0;
  int incl = mine;
  for (int o = 1; o < 64; o <<= 1) {
    const int up = __shfl_up(incl, o);
    if (lane >= o) incl += up;
  }
  if (lane == 63) wave_off[wave] = incl;
  __syncthreads();
  int first = incl - mine;
  for (int w = 0; w < wave; ++w) first += wave_off[w];
  const int n = wave_off[0] + wave_off[1] + wave_off[2] + wave_off[3];  // n_tail <= M < kPsisTail
  {
    int pos = first;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
      const int d = i * kPsisThreads + tid;
      const double x = psis_unkey(key[i]);
      if (d < S && x > cut) {
        if (pos < kPsisTail) {
          tail_v[pos] = x;
          tail_p[pos] = ((uint32_t)d << 9) | (uint32_t)pos;
        }
        ++pos;
      }
    }
  }

  double pareto_k = INFINITY;
  const bool smoothed = n > 4 && n <= kPsisTail;
  if (smoothed) {  // the whole block
    int P = 8;
    while (P < n) P <<= 1;
    for (int i = n + tid; i < P; i += kPsisThreads) {
      tail_v[i] = INFINITY;
      tail_p[i] = 0xffffffffu;
    }
    __syncthreads();
    for (int k2 = 2; k2 <= P; k2 <<= 1)
      for (int j = k2 >> 1; j > 0; j >>= 1) {
        for (int t = tid; t < (P >> 1); t += kPsisThreads) {
          const int lo = ((t & ~(j - 1)) << 1) | (t & (j - 1)), hi = lo | j;
          const double vl = tail_v[lo], vh = tail_v[hi];
          const uint32_t pl = tail_p[lo], p_h = tail_p[hi];
          const bool gt = vl > vh || (vl == vh && pl > p_h);
          if (gt == ((lo & k2) == 0)) {
            tail_v[lo] = vh;
            tail_v[hi] = vl;
            tail_p[lo] = p_h;
            tail_p[hi] = pl;
          }
        }
        __syncthreads();
      }
    // 4. the fit
    for (int i = tid; i < n; i += kPsisThreads) tail_v[i] = exp(tail_v[i]) - ecut;
    __syncthreads();
    const double dn = (double)n;
    const int m = 30 + (int)floor(sqrt(dn));
    const double t_q = tail_v[(int)(dn / 4.0 + 0.5) - 1], t_max = tail_v[n - 1];
    for (int j = wave + 1; j <= m; j += 4) {
      const double bj = (1.0 - sqrt((double)m / ((double)j - 0.5))) / (3.0 * t_q) + 1.0 / t_max;
      double s = 0.0;
      for (int i = lane; i < n; i += 64) s += log1p(-bj * tail_v[i]);
      const double kj = psis_wave_reduce(s, PsisSum()) / dn;
      if (lane == 0) {
        grid_b[j - 1] = bj;
        grid_l[j - 1] = dn * (log(-bj / kj) - kj - 1.0);
      }
    }
    __syncthreads();
    if (tid < m) {
      const double lj = grid_l[tid];
      double s = 0.0;
      for (int i = 0; i < m; ++i) s += exp(grid_l[i] - lj);
      grid_w[tid] = 1.0 / s;
    }
    __syncthreads();
    double b = 0.0;
    for (int j = 0; j < m; ++j) b += grid_b[j] * grid_w[j];
    double s = 0.0;
    for (int i = lane; i < n; i += 64) s += log1p(-b * tail_v[i]);
    const double k_raw = psis_wave_reduce(s, PsisSum()) / dn;  // every wave the same bits
    const double sigma = -k_raw / b;
    pareto_k = (dn * k_raw + 5.0) / (dn + 10.0);
    // 5. the smoothed tail, by compaction index
    for (int i = tid; i < n; i += kPsisThreads) {
      const double lp = log1p(-((double)i + 0.5) / dn);
      const double q = pareto_k == 0.0 ? -sigma * lp : sigma * expm1(-pareto_k * lp) / pareto_k;
      smooth[tail_p[i] & 511u] = fmin(log(q + ecut), 0.0);
    }
    __syncthreads();
  }

  // 6. the weights and elpd_loo.  xw(i, pos): draw i's smoothed x, pos the running compaction index
  auto xw = [&](int i, int& pos) {
    const double x = psis_unkey(key[i]);
    if (x > cut) {
      const int p = pos++;
      if (smoothed) return smooth[p];
    }
    return x;
  };
  double mx = -INFINITY;
  {
    int pos = first;
#pragma unroll
    for (int i = 0; i < VPT; ++i)
      if (i * kPsisThreads + tid < S) mx = fmax(mx, xw(i, pos));
  }
  mx = psis_block_reduce(mx, PsisMax(), red_d, ph_d);
  double sx = 0.0;
  {
    int pos = first;
#pragma unroll
    for (int i = 0; i < VPT; ++i)
      if (i * kPsisThreads + tid < S) sx += exp(xw(i, pos) - mx);
  }
  sx = psis_block_reduce(sx, PsisSum(), red_d, ph_d);
  const double lse_x = mx + log(sx);
  double mv = -INFINITY;
  {
    int pos = first;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
      const int d = i * kPsisThreads + tid;
      if (d < S) mv = fmax(mv, row[d] + (xw(i, pos) - lse_x));
    }
  }
  mv = psis_block_reduce(mv, PsisMax(), red_d, ph_d);
  double sv = 0.0;
  {
    int pos = first;
#pragma unroll
    for (int i = 0; i < VPT; ++i) {
      const int d = i * kPsisThreads + tid;
      if (d < S) sv += exp((row[d] + (xw(i, pos) - lse_x)) - mv);
    }
  }
  sv = psis_block_reduce(sv, PsisSum(), red_d, ph_d);
  if (tid == 0) {
    a.elpd[unit] = mv + log(sv);
    a.lppd[unit] = lppd;
    a.pareto_k[unit] = pareto_k;
    a.n_tail[unit] = n;
  }
}

// The launch over S draws, for every caller alike: the arguments -- out [3][ld]: elpd_loo, pareto k, lppd -- with M, log S and
// log DBL_MIN from the host, and the kernel: the draws a thread holds in registers are the smallest of 1, 4, 16, 64 with
// S <= 256 VPT.  One workgroup of kPsisThreads per unit.
using PsisKernel = void (*)(const PsisArgs);
struct PsisLaunch {
  PsisKernel kernel;
  PsisArgs args;
};
inline PsisLaunch psis_launch(const double* mat, const int32_t* n_cells, double* out, int32_t* n_tail, size_t ld, int64_t capacity, int64_t S) {
  PsisArgs a;
  std::memset(&a, 0, sizeof a);
  a.mat = mat;
  a.n_cells = n_cells;
  a.elpd = out;
  a.pareto_k = out + ld;
  a.lppd = out + 2 * ld;
  a.n_tail = n_tail;
  a.capacity = capacity;
  a.S = (int32_t)S;
  a.M = psis_tail_len(S);
  a.log_S = std::log((double)S);
  a.log_tiny = std::log(std::numeric_limits<double>::min());
  const PsisKernel k = a.S <= 256 ? abd_psis_kernel<1> : a.S <= 1024 ? abd_psis_kernel<4> : a.S <= 4096 ? abd_psis_kernel<16> : abd_psis_kernel<64>;
  return {k, a};
}

}  // namespace abdi
