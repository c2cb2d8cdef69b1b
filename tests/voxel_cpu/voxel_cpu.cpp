// voxel_cpu.cpp -- test-side restatement of the voxel-grid downsampling contract (include/s4p_voxel.h), independent of the
// library's path: a std::map from (iz, iy, ix) to the member lists, explicit loops for the two-level sum.  Built by
// tests/voxel_helpers.py with -ffp-contract=off.
#include <cmath>
#include <cstdint>
#include <map>
#include <tuple>
#include <vector>

namespace {

// the contract's sum of one channel of the members: blocks of 64 positions summed in order, the blocks' sums added in order
double two_level(const std::vector<int64_t>& mem, const float* col, int64_t stride) {
  const size_t c = mem.size();
  double S = 0.0;
  for (size_t b = 0; 64 * b < c; ++b) {
    const size_t e = 64 * b + 64 < c ? 64 * b + 64 : c;
    double s = double(col[mem[64 * b] * stride]);
    for (size_t j = 64 * b + 1; j < e; ++j) s += double(col[mem[j] * stride]);
    if (b == 0) S = s; else S += s;
  }
  return S;
}

}  // namespace

extern "C" {

// returns m, or -1 when an axis spans more than 2^21 voxels
int64_t voxel_cpu_downsample(const float* x, const float* y, const float* z, int64_t n, float voxel, const float* attr, int32_t nattr,
                             float* out_xyz, float* out_attr, int32_t* out_count, int32_t* voxel_of) {
  const double v = double(voxel);
  std::map<std::tuple<double, double, double>, std::vector<int64_t>> cells;          // (iz, iy, ix) -> members, ascending index
  double lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  bool any = false;
  for (int64_t i = 0; i < n; ++i) {
    voxel_of[i] = -1;
    if (!std::isfinite(x[i]) || !std::isfinite(y[i]) || !std::isfinite(z[i])) continue;
    const double id[3] = {std::floor(double(x[i]) / v), std::floor(double(y[i]) / v), std::floor(double(z[i]) / v)};
    for (int a = 0; a < 3; ++a) {
      if (!any || id[a] < lo[a]) lo[a] = id[a];
      if (!any || id[a] > hi[a]) hi[a] = id[a];
    }
    any = true;
    cells[std::make_tuple(id[2], id[1], id[0])].push_back(i);
  }
  for (int a = 0; a < 3; ++a)
    if (any && !(hi[a] - lo[a] + 1.0 <= 2097152.0)) return -1;
  int64_t r = 0;
  for (const auto& kv : cells) {
    const std::vector<int64_t>& mem = kv.second;
    const double c = double(mem.size());
    out_xyz[3 * r] = float(two_level(mem, x, 1) / c);
    out_xyz[3 * r + 1] = float(two_level(mem, y, 1) / c);
    out_xyz[3 * r + 2] = float(two_level(mem, z, 1) / c);
    for (int32_t a = 0; a < nattr; ++a) out_attr[r * nattr + a] = float(two_level(mem, attr + a, nattr) / c);
    out_count[r] = int32_t(mem.size());
    for (int64_t i : mem) voxel_of[i] = int32_t(r);
    ++r;
  }
  return r;
}

}  // extern "C"
