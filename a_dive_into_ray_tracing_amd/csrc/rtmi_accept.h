// rtmi_accept.h — the root acceptance of the accelerated walks (rtmi_path.h
// resolve_root, resolve_key), in plain C++ so that a host program can call the
// very code the kernels run (tests/native/resolve_accept.cpp).
//
// sphere.h:30-38's root logic on the closed interval [0.001, t_max], with the
// order-independent tie rule: a root equal to t_max replaces the hit only for a
// later object.  The reference tries the near root r1 and, when it is refused,
// the far root r2.  Here ONE root is selected and tested once:
//   t = r1 >= 0.001 ? r1 : r2
// r1 <= r2 always holds (sq >= 0, inv_a >= 0, and the subtraction, the addition
// and the multiplication all round monotonically), so
//  - if r1 >= 0.001 and r1 is refused (beyond t_max, or a tie the earlier
//    object keeps), r2 >= r1 is refused for the same reason: r1 decides alone;
//  - if r1 < 0.001 or r1 is NaN (the ordered compare is false), the two-root
//    rule decides on r2 as well.
// Equal to the two-root rule for every input the kernels can form, NaN and
// +-inf roots included, given inv_a >= 0 or NaN and t_max = +inf or an accepted
// root (>= 0.001): tests/test_resolve_accept.py compares the two over 1e7
// random and special inputs, exact ties among them.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define RTMI_ACCEPT_FN __host__ __device__ __forceinline__
#else
#define RTMI_ACCEPT_FN inline
#endif

namespace rtmi {

// the two roots from hb = (o-c).d, sq = sqrt(disc) and inv_a = 1/(d.d)
RTMI_ACCEPT_FN void root_pair(float hb, float sq, float inv_a, float &r1, float &r2) {
  r1 = (-hb - sq) * inv_a;
  r2 = (-hb + sq) * inv_a;
}

// Accepts the selected root into t_max and says so.  later() tells whether
// this object comes after the one that holds t_max in scene order; it is
// called only for an exact tie (t == t_max), which is rare, so whatever it
// costs (a compare, two index reads) stays off the common path.
template <class Later>
RTMI_ACCEPT_FN bool accept_root(float r1, float r2, float &t_max, Later later) {
  const float t = r1 >= 0.001f ? r1 : r2;  // ordered: a NaN r1 falls to r2
  const bool in = !(t < 0.001f) & (t < t_max);
  bool ok = in;
  if (__builtin_expect(t == t_max, 0)) ok = later();  // `in` is false here
  if (ok) t_max = t;
  return ok;
}

}  // namespace rtmi
