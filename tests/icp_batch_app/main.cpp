// TopPoses (include/super4pcs/algorithms/icp_batch.h) as a plain host program: scripted arrival sequences against the
// entries they must leave.  Prints one line per check; exit status 0 only if every check holds.  Needs no device and no
// library (tests/test_icp_batch_host.py builds it as it is and once more with -fsanitize=address,undefined).
#include <cmath>
#include <cstdio>
#include <vector>

#include "super4pcs/algorithms/icp_batch.h"

using GlobalRegistration::TopPoses;

namespace {

int failures = 0;

void check(bool ok, const char* what) {
  std::printf("%s %s\n", ok ? "ok  " : "FAIL", what);
  if (!ok) ++failures;
}

// rotation by deg about z, then the translation (tx, ty, tz)
void pose(double deg, double tx, double ty, double tz, double M[16]) {
  const double a = deg * (3.14159265358979323846 / 180.0), c = std::cos(a), s = std::sin(a);
  const double R[16] = {c, -s, 0, tx, s, c, 0, ty, 0, 0, 1, tz, 0, 0, 0, 1};
  for (int k = 0; k < 16; ++k) M[k] = R[k];
}

struct Want { double lcp; double deg; };

bool holds(const TopPoses& top, const std::vector<Want>& want) {
  const auto& e = top.entries();
  if (e.size() != want.size()) return false;
  for (size_t i = 0; i < want.size(); ++i) {
    double M[16];
    pose(want[i].deg, 0, 0, 0, M);
    if (e[i].lcp != want[i].lcp || e[i].M[0] != M[0] || e[i].M[1] != M[1]) return false;
  }
  return true;
}

void add(const TopPoses& top, double lcp, double deg, double tx = 0, double ty = 0, double tz = 0) {
  double M[16];
  pose(deg, tx, ty, tz, M);
  top.Add(lcp, M);
}

}  // namespace

int main() {
  const double origin[3] = {0, 0, 0};
  {
    // a scripted sequence: K = 3, clusters 10 degrees / 0.5 wide around 0, 40, 80, 120 degrees
    TopPoses top(3, 10.0, 0.5, origin);
    add(top, 0.30, 0);
    add(top, 0.50, 40);
    add(top, 0.40, 80);
    check(holds(top, {{0.50, 40}, {0.40, 80}, {0.30, 0}}), "three distinct poses, sorted by LCP descending");
    add(top, 0.45, 3);                               // the cluster of 0 degrees, greater: replaces it and moves up
    check(holds(top, {{0.50, 40}, {0.45, 3}, {0.40, 80}}), "a greater LCP replaces its cluster's entry");
    add(top, 0.45, -2);                              // the same cluster (5 degrees from 3), equal LCP: kept out
    add(top, 0.44, 1);
    check(holds(top, {{0.50, 40}, {0.45, 3}, {0.40, 80}}), "an equal or smaller LCP inside a cluster changes nothing");
    add(top, 0.40, 120);                             // a new cluster at the smallest LCP: the tie keeps the earlier arrival
    check(holds(top, {{0.50, 40}, {0.45, 3}, {0.40, 80}}), "eviction needs a strictly greater LCP: a tie keeps the earlier arrival");
    add(top, 0.41, 120);
    check(holds(top, {{0.50, 40}, {0.45, 3}, {0.41, 120}}), "a new cluster with a greater LCP evicts the smallest");
    add(top, 0.45, 160);                             // equal to an entry: behind it (stable by arrival), 0.41 leaves
    check(holds(top, {{0.50, 40}, {0.45, 3}, {0.45, 160}}), "equal LCPs stay in the order of arrival");
    add(top, 0.10, 200);
    check(holds(top, {{0.50, 40}, {0.45, 3}, {0.45, 160}}), "a smaller LCP than every entry is dropped");
    check(top.arrivals() == 10, "every candidate is counted");
  }
  {
    // the angle test either side of 10 degrees
    TopPoses top(4, 10.0, 0.5, origin);
    add(top, 0.5, 0);
    add(top, 0.4, 9.99);
    check(top.entries().size() == 1, "9.99 degrees apart: the same pose");
    add(top, 0.4, 10.01);
    check(top.entries().size() == 2, "10.01 degrees apart: another pose");
    add(top, 0.3, -9.99);
    check(top.entries().size() == 2, "-9.99 degrees: the same pose as 0");
  }
  {
    // the centroid test either side of dist_tol, at equal rotations; the centroid is (1, 2, 3)
    const double c[3] = {1, 2, 3};
    TopPoses top(4, 10.0, 0.5, c);
    add(top, 0.5, 30);
    add(top, 0.4, 30, 0.49, 0, 0);
    check(top.entries().size() == 1, "centroid images 0.49 apart: the same pose");
    add(top, 0.4, 30, 0, 0.51, 0);
    check(top.entries().size() == 2, "centroid images 0.51 apart: another pose");
    // a rotation within the angle tolerance that carries the centroid farther than dist_tol: another pose
    TopPoses far(4, 10.0, 0.05, c);
    add(far, 0.5, 0);
    add(far, 0.4, 5);                                // (1, 2, 3) turned by 5 degrees about z moves by 0.195
    check(far.entries().size() == 2, "both conditions must hold");
    double A[16], B[16];
    pose(0, 0, 0, 0, A); pose(5, 0, 0, 0, B);
    check(!far.Same(A, B) && top.Same(A, B), "Same() is the conjunction");
  }
  {
    // K = 1 keeps the best distinct pose; the visitor interface takes per-candidate calls only
    TopPoses top(1, 10.0, 0.5, origin);
    GlobalRegistration::Match4PCSBase::MatrixType M;
    for (int r = 0; r < 4; ++r) for (int c = 0; c < 4; ++c) M(r, c) = float(r == c);
    top(0.5f, 0.9f, M);                              // a progress call
    check(top.entries().empty() && top.needsGlobalTransformation(), "progress calls are not candidates");
    top(-1.f, 0.25f, M);
    add(top, 0.2, 90);
    add(top, 0.3, 180);
    check(top.entries().size() == 1 && top.entries()[0].lcp == 0.3, "K = 1");
    const auto starts = top.StartsAfter(M);
    check(starts.size() == 1 && starts[0](0, 0) == 1.f && starts[0](0, 3) == 0.f, "the first start is the identity, at most K starts");
    TopPoses two(2, 10.0, 0.5, origin);
    add(two, 0.5, 90, 1, 0, 0);
    add(two, 0.4, 0);
    const auto s2 = two.StartsAfter(M);              // M is the identity: the entry at 0 degrees is its cluster and is skipped
    check(s2.size() == 2 && std::fabs(s2[1](0, 1) + 1.f) < 1e-6f && s2[1](0, 3) == 1.f, "the other starts are entries outside the result's cluster");
  }
  std::printf("%d failures\n", failures);
  return failures ? 1 : 0;
}
