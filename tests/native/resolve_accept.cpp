// tests/native/resolve_accept.cpp — the one-root acceptance of the accelerated
// walks (a_dive_into_ray_tracing_amd/csrc/rtmi_accept.h, the code the kernels
// run) against the literal two-root rule of sphere.h:30-38 with the
// order-independent tie rule, written out below.  Host only, its own main;
// built and run by tests/test_resolve_accept.py.
//
// Inputs: (hb, disc >= 0, a, t_max, later); sq = sqrtf(disc), inv_a = 1 / a,
// the roots by rtmi_accept.h's root_pair for both rules.  What the kernels can
// form: a = d.d >= 0 (so inv_a >= 0, +inf or NaN), t_max = +inf or a root
// accepted earlier (so t_max >= 0.001).
//  1. N random tuples (argv[1], fixed seed): magnitudes log-uniform over wide
//     ranges, signs of hb random; t_max random in [0.001, 1e4] or +inf, and
//     for every tuple also forced to r1, to r2 (where they are acceptable
//     roots, >= 0.001 and not NaN) and to +inf: the forcing makes the exact ties;
//  2. the full product of the special values +-0, 0.001f and its two
//     neighbours, denormals, +-inf, NaN, 3.4e38 (and a few ordinary ones) for
//     hb, sq and inv_a, with every admissible special t_max and the same forcing.
// Prints one line: cases, ties, accepted, differences.  Exit status 1 on any difference.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../a_dive_into_ray_tracing_amd/csrc/rtmi_accept.h"

static uint32_t bits(float x) {
  uint32_t u;
  memcpy(&u, &x, 4);
  return u;
}
static float from_bits(uint32_t u) {
  float x;
  memcpy(&x, &u, 4);
  return x;
}

// the two-root rule, literally: the near root if it lies in [0.001, t_max] (a
// tie with t_max counting only for a later object), else the far root likewise
static bool two_root_rule(float r1, float r2, bool later, float &t_max) {
  const bool ok1 = (!(r1 < 0.001f)) & ((r1 < t_max) | ((r1 == t_max) & later));
  const bool ok2 = (!(r2 < 0.001f)) & ((r2 < t_max) | ((r2 == t_max) & later));
  if (ok1 || ok2) {
    t_max = ok1 ? r1 : r2;
    return true;
  }
  return false;
}

struct Tally {
  unsigned long long cases = 0, ties = 0, accepted = 0, diffs = 0, later_calls_off_tie = 0;
};

static void one_case(float r1, float r2, float t_max, bool later, Tally &T) {
  float ta = t_max, tb = t_max;
  const bool want = two_root_rule(r1, r2, later, ta);
  bool called = false;
  const bool got = rtmi::accept_root(r1, r2, tb, [&] {
    called = true;
    return later;
  });
  T.cases++;
  // an exact tie exercised: the root the rule decides on equals t_max
  const float t = r1 >= 0.001f ? r1 : r2;
  const bool tie = t == t_max;
  T.ties += tie;
  T.accepted += want;
  if (called && !tie) T.later_calls_off_tie++;
  if (want != got || bits(ta) != bits(tb)) {
    if (T.diffs < 10)
      fprintf(stderr, "differs: r1 %a (%08x) r2 %a (%08x) t_max %a later %d: want %d %08x got %d %08x\n", r1, bits(r1), r2,
              bits(r2), t_max, int(later), int(want), bits(ta), int(got), bits(tb));
    T.diffs++;
  }
}

// a tuple under every t_max: the given one, r1 and r2 where they are roots that could have been accepted, +inf
static void tuple(float hb, float sq, float inv_a, float t_max, Tally &T) {
  float r1, r2;
  rtmi::root_pair(hb, sq, inv_a, r1, r2);
  for (int later = 0; later < 2; later++) {
    one_case(r1, r2, t_max, later, T);
    if (r1 >= 0.001f) one_case(r1, r2, r1, later, T);
    if (r2 >= 0.001f) one_case(r1, r2, r2, later, T);
    one_case(r1, r2, INFINITY, later, T);
  }
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t next_u64() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}
static double uniform() { return double(next_u64() >> 11) * 0x1p-53; }
static float log_uniform(double lo, double hi) { return float(exp(log(lo) + uniform() * (log(hi) - log(lo)))); }

int main(int argc, char **argv) {
  const unsigned long long n = argc > 1 ? strtoull(argv[1], nullptr, 10) : 10000000ull;
  Tally T;
  // 1. random tuples
  for (unsigned long long i = 0; i < n; i++) {
    const float a = log_uniform(1e-6, 1e6);
    float hb = log_uniform(1e-4, 1e4) * sqrtf(a);
    if (next_u64() & 1) hb = -hb;
    // disc from nothing (tangent) up to well beyond hb^2 (origins inside the sphere)
    const float disc = (next_u64() & 7) == 0 ? 0.0f : hb * hb * log_uniform(1e-8, 4.0);
    const float t_max = (next_u64() & 3) == 0 ? INFINITY : log_uniform(0.001, 1e4);
    tuple(hb, sqrtf(disc), 1.0f / a, t_max < 0.001f ? 0.001f : t_max, T);
  }
  // 2. the specials
  const float k = 0.001f;
  const std::vector<float> sp = {0.0f,      -0.0f,     k,         from_bits(bits(k) - 1), from_bits(bits(k) + 1), -k,
                                 1e-45f,    -1e-45f,   1e-39f,    -1e-39f,                INFINITY,               -INFINITY,
                                 NAN,       3.4e38f,   -3.4e38f,  1.0f,                   -1.0f,                  0.5f,
                                 2.0f,      1e-3f * 2, 0.0005f,   -0.0005f,               1e20f,                  1e-20f};
  std::vector<float> sq_sp, inv_sp, tm_sp;
  for (float v : sp) {
    if (!(v < 0.0f) && bits(v) != bits(-0.0f)) sq_sp.push_back(v), inv_sp.push_back(v);  // >= +0, or NaN
    if (v >= 0.001f) tm_sp.push_back(v);                                                  // an accepted root, or +inf
  }
  for (float hb : sp)
    for (float sq : sq_sp)
      for (float inv_a : inv_sp)
        for (float t_max : tm_sp) tuple(hb, sq, inv_a, t_max, T);
  printf("{\"cases\": %llu, \"ties\": %llu, \"accepted\": %llu, \"later_calls_off_tie\": %llu, \"differences\": %llu}\n", T.cases, T.ties,
         T.accepted, T.later_calls_off_tie, T.diffs);
  return T.diffs != 0;
}
