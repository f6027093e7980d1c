// CPU harness for the step function of abd_simulate.hpp (tests/test_simulation_cpu.py): the walk of the cohort simulator, gap
// after gap, with the keyed Philox draws the kernel makes or with injected uniforms, and the OD of a reading.  The kernel
// compiles the same sim_step / sim_od.  With -DSIM_HARNESS_MAIN it is a stand-alone program for the sanitizers.
#include <cstdio>
#include <vector>

#include "abd_simulate.hpp"

using namespace abdi;

namespace {

// par: protect_a, protect_b, init, perm_rise, temp_rise_i, temp_rise_v, temp_wane of S, then of N (SimWalkAb's order)
SimWalkPar walk_par(const double* par) {
  SimWalkPar p;
  p.s = {par[0], par[1], par[2], par[3], par[4], par[5], par[6]};
  p.n = {par[7], par[8], par[9], par[10], par[11], par[12], par[13]};
  return p;
}

struct Injected {  // row j of (N, G) arrays of uniforms
  const double *u_e, *u_s, *u_n;
  double exposure(uint32_t t) const { return u_e[t]; }
  void protection(uint32_t t, double& us, double& un) const {
    us = u_s[t];
    un = u_n[t];
  }
};

template <typename Draws>
void walk_one(const SimWalkPar& p, const double* lam0, const int8_t* vacs, const int8_t* pcrpos, int G, const Draws& dr, int8_t* inf,
              double* s, double* n) {
  SimState st = sim_start(p);
  for (int t = 0; t < G; ++t) {
    inf[t] = sim_step(p, st, lam0[t], pcrpos && pcrpos[t] == 1, vacs[t] == 1, dr, (uint32_t)t) ? 1 : 0;
    s[t] = st.s_prev;
    n[t] = st.n_prev;
  }
}

}  // namespace

// vacs, pcrpos (may be NULL), inf, s, n: (N, G) row-major
extern "C" void sim_walk_keyed(const double* par, const double* lam0, const int8_t* vacs, const int8_t* pcrpos, int N, int G,
                               uint64_t seed, uint32_t rho, uint32_t ind_offset, int8_t* inf, double* s, double* n) {
  const SimWalkPar p = walk_par(par);
  for (int j = 0; j < N; ++j) {
    const size_t o = (size_t)j * G;
    const SimKeyed dr{(uint32_t)seed, (uint32_t)(seed >> 32), ind_offset + (uint32_t)j, rho};
    walk_one(p, lam0, vacs + o, pcrpos ? pcrpos + o : nullptr, G, dr, inf + o, s + o, n + o);
  }
}

extern "C" void sim_walk_injected(const double* par, const double* lam0, const int8_t* vacs, const int8_t* pcrpos, int N, int G,
                                  const double* u_e, const double* u_s, const double* u_n, int8_t* inf, double* s, double* n) {
  const SimWalkPar p = walk_par(par);
  for (int j = 0; j < N; ++j) {
    const size_t o = (size_t)j * G;
    walk_one(p, lam0, vacs + o, pcrpos ? pcrpos + o : nullptr, G, Injected{u_e + o, u_s + o, u_n + o}, inf + o, s + o, n + o);
  }
}

extern "C" void sim_keyed_uniforms(int N, int G, uint64_t seed, uint32_t rho, uint32_t ind_offset, double* u_e, double* u_s, double* u_n) {
  for (int j = 0; j < N; ++j) {
    const SimKeyed dr{(uint32_t)seed, (uint32_t)(seed >> 32), ind_offset + (uint32_t)j, rho};
    for (int t = 0; t < G; ++t) {
      u_e[(size_t)j * G + t] = dr.exposure((uint32_t)t);
      dr.protection((uint32_t)t, u_s[(size_t)j * G + t], u_n[(size_t)j * G + t]);
    }
  }
}

extern "C" void sim_od_row(double b, double d, double sd, const double* log_dilution, const double* titer, const double* z, int K, double* od) {
  for (int k = 0; k < K; ++k) od[k] = sim_od(b, d, sd, log_dilution[k], titer[k], z[k]);
}

#ifdef SIM_HARNESS_MAIN
// Keyed walks against the walk fed the same uniforms, at sizes around the 64-gap words, with and without PCR positives.
int main() {
  const double par[14] = {0.3, 1.7, -1.0, 0.34, 0.3, 0.21, 0.94, -0.2, 0.8, -2.0, 2.34, 0.89, 0.0, 0.87};
  uint64_t lcg = 12345;
  auto rnd = [&] { return (double)((lcg = lcg * 6364136223846793005ull + 1442695040888963407ull) >> 11) / 9007199254740992.0; };
  for (const int G : {1, 5, 63, 64, 65, 300}) {
    const int N = 37;
    const size_t c = (size_t)N * G;
    std::vector<double> lam((size_t)G), ue(c), us(c), un(c), s1(c), n1(c), s2(c), n2(c), od(c), z(c, 0.25);
    std::vector<int8_t> v(c), pc(c), i1(c), i2(c);
    for (auto& x : lam) x = 0.5 * rnd();
    for (size_t k = 0; k < c; ++k) {
      v[k] = rnd() < 0.05;
      pc[k] = rnd() < 0.03;
    }
    for (const int8_t* pcr : {(const int8_t*)pc.data(), (const int8_t*)nullptr}) {
      sim_walk_keyed(par, lam.data(), v.data(), pcr, N, G, 0xFEDCBA9876543210ull, 0x80000005u, 0xFFFFFFF0u, i1.data(), s1.data(), n1.data());
      sim_keyed_uniforms(N, G, 0xFEDCBA9876543210ull, 0x80000005u, 0xFFFFFFF0u, ue.data(), us.data(), un.data());
      sim_walk_injected(par, lam.data(), v.data(), pcr, N, G, ue.data(), us.data(), un.data(), i2.data(), s2.data(), n2.data());
      long n_inf = 0;
      for (size_t k = 0; k < c; ++k) {
        if (i1[k] != i2[k] || s1[k] != s2[k] || n1[k] != n2[k]) return std::printf("G=%d: keyed and injected walks differ at %zu\n", G, k), 1;
        if (!(ue[k] > 0.0 && ue[k] < 1.0 && us[k] > 0.0 && us[k] < 1.0 && un[k] > 0.0 && un[k] < 1.0)) return std::printf("uniform outside (0, 1)\n"), 1;
        if (pcr && pcr[k] && !i1[k]) return std::printf("a PCR+ is not an infection\n"), 1;
        n_inf += i1[k];
      }
      sim_od_row(-2.2, 1.6, 0.1, s1.data(), n1.data(), z.data(), (int)c, od.data());
      for (size_t k = 0; k < c; ++k)
        if (!(od[k] > 0.0 && od[k] < 1.7)) return std::printf("od out of range\n"), 1;
      std::printf("G=%d pcr=%d infections=%ld\n", G, pcr != nullptr, n_inf);
    }
  }
  std::puts("simulate ok");
  return 0;
}
#endif
