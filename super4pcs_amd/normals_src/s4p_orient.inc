// s4p_orient.inc -- consistent orientation of normals in libsuper4pcs_normals.so (include/s4p_normals_orient.h, DESIGN.md
// section 26).  Included by s4p_normals.hip after s4p_knn.inc: the functions work on an s4p_normals_ctx after set_cloud, on
// its cloud, grid, stream and arena.
//
// Device path (Boruvka's minimum spanning forest with parity-carrying pointer jumping; every phase is a kernel of its own,
// so kernel boundaries are the only ordering between workgroups):
//   lists     k_knn_search<K, kLists> with exclude_self, into the arena.
//   edges     k_orient_edges: a lane per point; the label word of the point (parent << 1 | parity, itself and 0 at the start;
//             ~0 for a point that is no vertex) and the bits of w of each of its k list entries (~0: no edge).
//   rounds    k_orient_min<0>: every entry whose ends carry different labels proposes (w bits << 32 | min(i, j)) to both
//             ends' components by a 64-bit atomicMin; k_orient_min<1>: the entries that tie with the winner propose
//             max(i, j) by a 32-bit atomicMin.  The lane's own side is reduced over its k entries and then over the wave's runs
//             of equal labels (points come in cell order, so neighbouring lanes mostly share a label); every atomic is
//             skipped when a plain load already shows a value that is not larger (the word only ever decreases).  A point
//             none of whose entries leaves its component is marked and passed over in every later round (components only
//             merge), so the rounds after the first few touch the components' borders only.
//             k_orient_hook: each root hooks onto the root of its edge's other end (a mutual pick keeps the hook of the
//             larger root index only) and counts itself; it reads one label array and writes the other.
//             k_orient_jump: label[v] = label[label[v]] with the parities XORed, from one array into the other, until a
//             launch reports that nothing moved: every round starts from stars.
//             The host reads one word per launch it waits for and bounds both loops (S4P_ORIENT_MAX_ROUNDS / _JUMPS).
//   anchor    k_orient_anchor: one 64-bit atomicMin per run of equal labels per wave on (d2 bits, index) (viewpoint) or
//             (~d2 bits, index) (outward); k_orient_anchor_flip: per root, the anchor's own flip XOR its parity.
//   apply     k_orient_apply: the final flip bit, the normals, flipped, component; the flipped count is an integer atomic.
// No float or double atomics; the only sums are integer counts.

#include "s4p_normals_orient.h"

namespace s4p_nrm {

static_assert(S4P_ORIENT_ERR_INTERNAL == kErrInternal, "arena_layout fails with the family's internal code");
constexpr uint32_t kNoLabel = 0xFFFFFFFFu;      // label word of a point that is no vertex (a parent is at most 2^31 - 3)
constexpr uint32_t kNoEdge = 0xFFFFFFFFu;       // w bits of a list entry that is no edge (w <= 1.0f = 0x3F800000)
enum OrientCount { kCntVertices = 0, kCntComponents = 1, kCntFlipped = 2, kCntMerged = 3, kCntChanged = 4, kCntWords = 8 };

__device__ inline float dot3(float ax, float ay, float az, float bx, float by, float bz) { return ax * bx + (ay * by + az * bz); }
__device__ inline bool usable_normal(float x, float y, float z) {
  return isfinite(x) && isfinite(y) && isfinite(z) && !(x == 0.f && y == 0.f && z == 0.f);
}

// Every lane of the wave calls this (a lane with nothing to propose passes label kNoLabel and key ~0).  Returns true in the
// last lane of each run of equal labels, whose key is then the minimum over the run.
__device__ inline bool wave_run_min(uint32_t label, uint64_t& key) {
  const int lane = int(threadIdx.x & 63u);
#pragma unroll
  for (int off = 1; off < 64; off <<= 1) {
    const uint32_t ol = __shfl_up(label, off, 64);
    const uint32_t klo = __shfl_up(uint32_t(key), off, 64), khi = __shfl_up(uint32_t(key >> 32), off, 64);
    const uint64_t ok = uint64_t(khi) << 32 | klo;
    if (lane >= off && ol == label && ok < key) key = ok;
  }
  const uint32_t nl = __shfl_down(label, 1, 64);
  return lane == 63 || nl != label;
}

// atomicMin that is skipped when the word already holds a value that is not larger (it only ever decreases)
__device__ inline void min64(unsigned long long* p, uint64_t key) {
  if (key < *(volatile unsigned long long*)p) atomicMin(p, (unsigned long long)key);
}
__device__ inline void min32(uint32_t* p, uint32_t v) {
  if (v < *(volatile uint32_t*)p) atomicMin(p, v);
}

// a lane per point (cell order): its label word, and w of each list entry
__global__ __launch_bounds__(kBlock) void k_orient_edges(const float4* pts, uint64_t n, int32_t k, const int32_t* idx, const float* nrm,
                                                         uint32_t* wbits, uint32_t* label, uint8_t* live, uint32_t* cnt) {
  for (uint64_t s = blockIdx.x * (uint64_t)kBlock + threadIdx.x; s < n; s += (uint64_t)gridDim.x * kBlock) {
    const uint32_t i = __float_as_uint(pts[s].w);
    const float nx = nrm[3ull * i], ny = nrm[3ull * i + 1], nz = nrm[3ull * i + 2];
    const bool v = usable_normal(nx, ny, nz);
    label[i] = v ? i << 1 : kNoLabel;
    live[i] = v ? 1 : 0;
    if (v) atomicAdd(&cnt[kCntVertices], 1u);
    for (int t = 0; t < k; ++t) {
      const uint64_t e = uint64_t(i) * uint64_t(k) + uint64_t(t);
      const int32_t j = idx[e];
      uint32_t w = kNoEdge;
      if (v && j >= 0) {
        const float mx = nrm[3ull * uint32_t(j)], my = nrm[3ull * uint32_t(j) + 1], mz = nrm[3ull * uint32_t(j) + 2];
        if (usable_normal(mx, my, mz)) {
          const float d = dot3(nx, ny, nz, mx, my, mz);
          const float t1 = 1.f - fabsf(d);
          w = __float_as_uint(t1 > 0.f ? t1 : 0.f);
        }
      }
      wbits[e] = w;
    }
  }
}

// PASS 0: best[c] = min (w bits << 32 | min(i, j)) over the entries that leave component c; PASS 1: among the entries that
// tie with best[c], besthi[c] = min max(i, j).  The block's trips are uniform, so every lane reaches wave_run_min.
template <int PASS>
__global__ __launch_bounds__(kBlock) void k_orient_min(const float4* pts, uint64_t n, int32_t k, const int32_t* idx, const uint32_t* wbits,
                                                       const uint32_t* label, uint8_t* live, unsigned long long* best, uint32_t* besthi) {
  for (uint64_t base = blockIdx.x * (uint64_t)kBlock; base < n; base += (uint64_t)gridDim.x * kBlock) {
    const uint64_t s = base + threadIdx.x;
    uint32_t ci = kNoLabel;
    uint64_t own = ~0ull;
    if (s < n) {
      const uint32_t i = __float_as_uint(pts[s].w);
      if (live[i]) {                                        // a vertex with an entry that left its component last round
        ci = label[i] >> 1;
        uint32_t pend = kNoLabel;                           // the other side, flushed when its component changes
        uint64_t pkey = ~0ull;
        for (int t = 0; t < k; ++t) {
          const uint64_t e = uint64_t(i) * uint64_t(k) + uint64_t(t);
          const uint32_t w = wbits[e];
          if (w == kNoEdge) continue;
          const uint32_t j = uint32_t(idx[e]);
          const uint32_t cj = label[j] >> 1;
          if (cj == ci) continue;
          const uint64_t key = uint64_t(w) << 32 | (i < j ? i : j);
          if (PASS == 0) {
            own = key < own ? key : own;
            if (cj != pend) {
              if (pend != kNoLabel) min64(&best[pend], pkey);
              pend = cj; pkey = key;
            } else {
              pkey = key < pkey ? key : pkey;
            }
          } else {
            const uint32_t hi = i < j ? j : i;
            if (best[ci] == key) min32(&besthi[ci], hi);
            if (best[cj] == key) min32(&besthi[cj], hi);
          }
        }
        if (PASS == 0 && pend != kNoLabel) min64(&best[pend], pkey);
        if (PASS == 0 && own == ~0ull) live[i] = 0;         // only this lane writes live[i]
      }
    }
    if (PASS == 0) {
      const uint32_t lab = own == ~0ull ? kNoLabel : ci;
      if (wave_run_min(lab, own) && lab != kNoLabel) min64(&best[lab], own);
    }
  }
}

// Every root with an edge hooks onto the root of the edge's other end; everything else is copied.  in -> out.
__global__ __launch_bounds__(kBlock) void k_orient_hook(uint64_t n, const uint32_t* in, uint32_t* out, const unsigned long long* best,
                                                        const uint32_t* besthi, const float* nrm, uint32_t* cnt) {
  for (uint64_t v = blockIdx.x * (uint64_t)kBlock + threadIdx.x; v < n; v += (uint64_t)gridDim.x * kBlock) {
    const uint32_t a = in[v];
    uint32_t o = a;
    if (a != kNoLabel && (a >> 1) == uint32_t(v)) {
      const unsigned long long key = best[v];
      if (key != ~0ull) {
        const uint32_t lo = uint32_t(key), hi = besthi[v];
        const uint32_t la = in[lo], lb = in[hi];
        const bool lo_mine = (la >> 1) == uint32_t(v);
        const uint32_t mine = lo_mine ? la : lb, other = lo_mine ? lb : la;
        const uint32_t rb = other >> 1;
        const bool mutual = best[rb] == key && besthi[rb] == hi;
        if (!(mutual && uint32_t(v) < rb)) {
          const float d = dot3(nrm[3ull * lo], nrm[3ull * lo + 1], nrm[3ull * lo + 2], nrm[3ull * hi], nrm[3ull * hi + 1], nrm[3ull * hi + 2]);
          const uint32_t f = d < 0.f ? 1u : 0u;
          o = rb << 1 | ((mine ^ other ^ f) & 1u);
          atomicAdd(&cnt[kCntMerged], 1u);
        }
      }
    }
    out[v] = o;
  }
}

// one step of pointer jumping with parity, in -> out
__global__ __launch_bounds__(kBlock) void k_orient_jump(uint64_t n, const uint32_t* in, uint32_t* out, uint32_t* cnt) {
  bool moved = false;
  for (uint64_t v = blockIdx.x * (uint64_t)kBlock + threadIdx.x; v < n; v += (uint64_t)gridDim.x * kBlock) {
    const uint32_t a = in[v];
    uint32_t o = a;
    if (a != kNoLabel) {
      const uint32_t b = in[a >> 1];
      o = (b & ~1u) | ((a ^ b) & 1u);
      moved |= (b >> 1) != (a >> 1);
    }
    out[v] = o;
  }
  if (moved) cnt[kCntChanged] = 1u;            // a flag: every writer stores the same value
}

// best[root] = min over the component of (d2 bits or their complement) << 32 | index, d2 to (px, py, pz)
__global__ __launch_bounds__(kBlock) void k_orient_anchor(const float4* pts, uint64_t n, const uint32_t* label, float px, float py, float pz,
                                                          uint32_t farthest, unsigned long long* best) {
  for (uint64_t base = blockIdx.x * (uint64_t)kBlock; base < n; base += (uint64_t)gridDim.x * kBlock) {
    const uint64_t s = base + threadIdx.x;
    uint32_t lab = kNoLabel;
    uint64_t key = ~0ull;
    if (s < n) {
      const float4 p = pts[s];
      const uint32_t i = __float_as_uint(p.w);
      const uint32_t li = label[i];
      if (li != kNoLabel) {
        lab = li >> 1;
        const float dx = p.x - px, dy = p.y - py, dz = p.z - pz;
        const uint32_t b = __float_as_uint(dx * dx + (dy * dy + dz * dz));
        key = uint64_t(farthest ? ~b : b) << 32 | i;
      }
    }
    if (wave_run_min(lab, key) && lab != kNoLabel) min64(&best[lab], key);
  }
}

// per root: rootflip[root] = (the anchor's own flip) XOR (the anchor's parity to the root)
__global__ __launch_bounds__(kBlock) void k_orient_anchor_flip(uint64_t n, const uint32_t* label, const unsigned long long* best,
                                                               const float4* pos, const float* nrm, float px, float py, float pz,
                                                               uint32_t farthest, uint32_t* rootflip, uint32_t* cnt) {
  for (uint64_t v = blockIdx.x * (uint64_t)kBlock + threadIdx.x; v < n; v += (uint64_t)gridDim.x * kBlock) {
    const uint32_t a = label[v];
    if (a == kNoLabel || (a >> 1) != uint32_t(v)) continue;
    const uint32_t anchor = uint32_t(best[v]);
    const float4 x = pos[anchor];
    const float gx = farthest ? x.x - px : px - x.x, gy = farthest ? x.y - py : py - x.y, gz = farthest ? x.z - pz : pz - x.z;
    const float d = dot3(nrm[3ull * anchor], nrm[3ull * anchor + 1], nrm[3ull * anchor + 2], gx, gy, gz);
    rootflip[v] = ((d < 0.f ? 1u : 0u) ^ label[anchor]) & 1u;
    atomicAdd(&cnt[kCntComponents], 1u);
  }
}

__global__ __launch_bounds__(kBlock) void k_orient_apply(uint64_t n, const uint32_t* label, const unsigned long long* best,
                                                         const uint32_t* rootflip, float* nrm, uint8_t* flipped, int32_t* component,
                                                         uint32_t* cnt) {
  for (uint64_t v = blockIdx.x * (uint64_t)kBlock + threadIdx.x; v < n; v += (uint64_t)gridDim.x * kBlock) {
    const uint32_t a = label[v];
    uint32_t f = 0u;
    int32_t comp = -1;
    if (a != kNoLabel) {
      const uint32_t r = a >> 1;
      f = (rootflip[r] ^ a) & 1u;
      comp = int32_t(uint32_t(best[r]));
      if (f) {
        nrm[3 * v] = -nrm[3 * v]; nrm[3 * v + 1] = -nrm[3 * v + 1]; nrm[3 * v + 2] = -nrm[3 * v + 2];
        atomicAdd(&cnt[kCntFlipped], 1u);
      }
    }
    if (flipped) flipped[v] = uint8_t(f);
    if (component) component[v] = comp;
  }
}

// the simple call: towards a viewpoint, point by point
__global__ __launch_bounds__(kBlock) void k_orient_towards(uint64_t n, const float4* pos, float px, float py, float pz, float* nrm,
                                                           uint8_t* flipped) {
  for (uint64_t v = blockIdx.x * (uint64_t)kBlock + threadIdx.x; v < n; v += (uint64_t)gridDim.x * kBlock) {
    const float nx = nrm[3 * v], ny = nrm[3 * v + 1], nz = nrm[3 * v + 2];
    const float4 x = pos[v];
    const bool f = usable_normal(nx, ny, nz) && dot3(nx, ny, nz, px - x.x, py - x.y, pz - x.z) < 0.f;
    if (f) { nrm[3 * v] = -nx; nrm[3 * v + 1] = -ny; nrm[3 * v + 2] = -nz; }
    if (flipped) flipped[v] = f ? 1 : 0;
  }
}

}  // namespace s4p_nrm

namespace {

int32_t orient_word(s4p_normals_ctx* h, const uint32_t* dev, uint32_t* out) {
  NRM_HIP(hipMemcpyAsync(out, dev, sizeof(uint32_t), hipMemcpyDeviceToHost, h->st));
  NRM_HIP(hipStreamSynchronize(h->st));
  return S4P_NORMALS_OK;
}

bool finite3(const float* v) { return v && std::isfinite(v[0]) && std::isfinite(v[1]) && std::isfinite(v[2]); }

int32_t orient_impl(s4p_normals_ctx* h, int32_t k, float radius, int32_t mode, const float* viewpoint, float* normals, uint8_t* flipped,
                    int32_t* component, s4p_orient_stats* stats, bool device) {
  if (!h) return S4P_NORMALS_ERR_BAD_ARG;
  if (int32_t rc = knn_check(h, "orient_consistent", k)) return rc;
  if (!std::isfinite(radius)) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "orient_consistent: radius must be finite (<= 0: unbounded)");
  if (mode != S4P_ORIENT_OUTWARD && mode != S4P_ORIENT_VIEWPOINT)
    return fail(h, S4P_NORMALS_ERR_BAD_ARG, "orient_consistent: mode must be S4P_ORIENT_OUTWARD or S4P_ORIENT_VIEWPOINT");
  if (mode == S4P_ORIENT_VIEWPOINT && !finite3(viewpoint))
    return fail(h, S4P_NORMALS_ERR_BAD_ARG, "orient_consistent: the viewpoint must be three finite floats");
  if (!normals) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "orient_consistent: null normals");
  NRM_HIP(hipSetDevice(h->device));
  const uint64_t un = uint64_t(h->n);
  const size_t nk = size_t(un) * size_t(k);
  const int nb = blocks_for(h->n);
  int32_t* idx = nullptr;
  float* d2 = nullptr;
  uint32_t *wbits = nullptr, *cur = nullptr, *nxt = nullptr, *besthi = nullptr, *cnt = nullptr;
  unsigned long long* best = nullptr;
  uint8_t* live = nullptr;
  float* dn = normals;
  uint8_t* dfl = flipped;
  int32_t* dco = component;
  if (int32_t rc = arena_layout(h, "orient_consistent", [&](Arena& ar) {
        idx = ar.take<int32_t>(nk);
        d2 = ar.take<float>(nk);
        wbits = ar.take<uint32_t>(nk);
        cur = ar.take<uint32_t>(un);
        nxt = ar.take<uint32_t>(un);
        besthi = ar.take<uint32_t>(un);
        best = ar.take<unsigned long long>(un);
        cnt = ar.take<uint32_t>(kCntWords);
        live = ar.take<uint8_t>(un);
        if (!device) {
          dn = ar.take<float>(3 * un);
          if (flipped) dfl = ar.take<uint8_t>(un);
          if (component) dco = ar.take<int32_t>(un);
        }
      })) return rc;
  if (!device) NRM_HIP(hipMemcpyAsync(dn, normals, 3 * un * sizeof(float), hipMemcpyHostToDevice, h->st));
  NRM_HIP(hipMemsetAsync(cnt, 0, kCntWords * 4, h->st));
  SearchArgs A{};
  A.qs = h->pts; A.m = un; A.k = k; A.self_mask = ~0u; A.idx = idx; A.d2 = d2; A.cnt = nullptr;
  if (int32_t rc = launch_search<kLists>(h, A, radius)) return rc;
  hipLaunchKernelGGL(k_orient_edges, dim3(nb), dim3(kBlock), 0, h->st, (const float4*)h->pts, un, k, (const int32_t*)idx, (const float*)dn,
                     wbits, cur, live, cnt);
  NRM_HIP(hipGetLastError());
  int32_t rounds = 0, max_jumps = 0;
  bool done = false;
  for (int r = 0; r < S4P_ORIENT_MAX_ROUNDS && !done; ++r) {
    NRM_HIP(hipMemsetAsync(best, 0xFF, un * 8, h->st));
    NRM_HIP(hipMemsetAsync(besthi, 0xFF, un * 4, h->st));
    NRM_HIP(hipMemsetAsync(cnt + kCntMerged, 0, 4, h->st));
    hipLaunchKernelGGL(k_orient_min<0>, dim3(nb), dim3(kBlock), 0, h->st, (const float4*)h->pts, un, k, (const int32_t*)idx,
                       (const uint32_t*)wbits, (const uint32_t*)cur, live, best, besthi);
    NRM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_orient_min<1>, dim3(nb), dim3(kBlock), 0, h->st, (const float4*)h->pts, un, k, (const int32_t*)idx,
                       (const uint32_t*)wbits, (const uint32_t*)cur, live, best, besthi);
    NRM_HIP(hipGetLastError());
    hipLaunchKernelGGL(k_orient_hook, dim3(nb), dim3(kBlock), 0, h->st, un, (const uint32_t*)cur, nxt, (const unsigned long long*)best,
                       (const uint32_t*)besthi, (const float*)dn, cnt);
    NRM_HIP(hipGetLastError());
    std::swap(cur, nxt);
    uint32_t merged = 0;
    if (int32_t rc = orient_word(h, cnt + kCntMerged, &merged)) return rc;
    if (merged == 0) { done = true; break; }
    ++rounds;
    int32_t jumps = 0;
    for (;;) {
      if (jumps == S4P_ORIENT_MAX_JUMPS)
        return fail(h, S4P_ORIENT_ERR_INTERNAL, "orient_consistent: pointer jumping did not reach stars within its bound (a cycle among the hooks)");
      NRM_HIP(hipMemsetAsync(cnt + kCntChanged, 0, 4, h->st));
      hipLaunchKernelGGL(k_orient_jump, dim3(nb), dim3(kBlock), 0, h->st, un, (const uint32_t*)cur, nxt, cnt);
      NRM_HIP(hipGetLastError());
      std::swap(cur, nxt);
      ++jumps;
      uint32_t changed = 0;
      if (int32_t rc = orient_word(h, cnt + kCntChanged, &changed)) return rc;
      if (!changed) break;
    }
    max_jumps = std::max(max_jumps, jumps);
  }
  if (!done) return fail(h, S4P_ORIENT_ERR_INTERNAL, "orient_consistent: components still merged after the last allowed round");
  float p[3];
  const uint32_t farthest = mode == S4P_ORIENT_OUTWARD ? 1u : 0u;
  for (int a = 0; a < 3; ++a) p[a] = farthest ? 0.5f * (h->lo[a] + h->hi[a]) : viewpoint[a];
  NRM_HIP(hipMemsetAsync(best, 0xFF, un * 8, h->st));
  hipLaunchKernelGGL(k_orient_anchor, dim3(nb), dim3(kBlock), 0, h->st, (const float4*)h->pts, un, (const uint32_t*)cur, p[0], p[1], p[2],
                     farthest, best);
  NRM_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_orient_anchor_flip, dim3(nb), dim3(kBlock), 0, h->st, un, (const uint32_t*)cur, (const unsigned long long*)best,
                     (const float4*)h->pos, (const float*)dn, p[0], p[1], p[2], farthest, besthi, cnt);
  NRM_HIP(hipGetLastError());
  hipLaunchKernelGGL(k_orient_apply, dim3(nb), dim3(kBlock), 0, h->st, un, (const uint32_t*)cur, (const unsigned long long*)best,
                     (const uint32_t*)besthi, dn, dfl, dco, cnt);
  NRM_HIP(hipGetLastError());
  uint32_t hc[kCntWords] = {};
  NRM_HIP(hipMemcpyAsync(hc, cnt, sizeof(hc), hipMemcpyDeviceToHost, h->st));
  if (!device) {
    NRM_HIP(hipMemcpyAsync(normals, dn, 3 * un * sizeof(float), hipMemcpyDeviceToHost, h->st));
    if (flipped) NRM_HIP(hipMemcpyAsync(flipped, dfl, un, hipMemcpyDeviceToHost, h->st));
    if (component) NRM_HIP(hipMemcpyAsync(component, dco, un * 4, hipMemcpyDeviceToHost, h->st));
  }
  NRM_HIP(hipStreamSynchronize(h->st));
  if (stats) {
    stats->vertices = hc[kCntVertices]; stats->components = hc[kCntComponents]; stats->flipped = hc[kCntFlipped];
    stats->rounds = rounds; stats->max_jumps = max_jumps;
  }
  return S4P_NORMALS_OK;
}

int32_t towards_impl(s4p_normals_ctx* h, float* normals, const float* viewpoint, uint8_t* flipped, bool device) {
  if (!h) return S4P_NORMALS_ERR_BAD_ARG;
  if (!h->has_cloud) return fail(h, S4P_NORMALS_ERR_STATE, "orient_towards: set_cloud first");
  if (!finite3(viewpoint)) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "orient_towards: the viewpoint must be three finite floats");
  if (!normals) return fail(h, S4P_NORMALS_ERR_BAD_ARG, "orient_towards: null normals");
  NRM_HIP(hipSetDevice(h->device));
  const uint64_t un = uint64_t(h->n);
  float* dn = normals;
  uint8_t* dfl = flipped;
  if (int32_t rc = arena_layout(h, "orient_towards", [&](Arena& ar) {
        if (device) return;
        dn = ar.take<float>(3 * un);
        if (flipped) dfl = ar.take<uint8_t>(un);
      })) return rc;
  if (!device) NRM_HIP(hipMemcpyAsync(dn, normals, 3 * un * sizeof(float), hipMemcpyHostToDevice, h->st));
  hipLaunchKernelGGL(k_orient_towards, dim3(blocks_for(h->n)), dim3(kBlock), 0, h->st, un, (const float4*)h->pos, viewpoint[0], viewpoint[1],
                     viewpoint[2], dn, dfl);
  NRM_HIP(hipGetLastError());
  if (!device) {
    NRM_HIP(hipMemcpyAsync(normals, dn, 3 * un * sizeof(float), hipMemcpyDeviceToHost, h->st));
    if (flipped) NRM_HIP(hipMemcpyAsync(flipped, dfl, un, hipMemcpyDeviceToHost, h->st));
  }
  NRM_HIP(hipStreamSynchronize(h->st));
  return S4P_NORMALS_OK;
}

}  // namespace

extern "C" {

int32_t s4p_orient_consistent(s4p_normals_ctx* h, int32_t k, float radius, int32_t mode, const float* viewpoint, float* normals,
                              uint8_t* flipped, int32_t* component, s4p_orient_stats* stats) {
  return orient_impl(h, k, radius, mode, viewpoint, normals, flipped, component, stats, false);
}
int32_t s4p_orient_consistent_device(s4p_normals_ctx* h, int32_t k, float radius, int32_t mode, const float* viewpoint,
                                     float* normals, uint8_t* flipped, int32_t* component, s4p_orient_stats* stats) {
  return orient_impl(h, k, radius, mode, viewpoint, normals, flipped, component, stats, true);
}

int32_t s4p_orient_towards(s4p_normals_ctx* h, float* normals, const float* viewpoint, uint8_t* flipped) {
  return towards_impl(h, normals, viewpoint, flipped, false);
}
int32_t s4p_orient_towards_device(s4p_normals_ctx* h, float* normals, const float* viewpoint, uint8_t* flipped) {
  return towards_impl(h, normals, viewpoint, flipped, true);
}

}  // extern "C"
