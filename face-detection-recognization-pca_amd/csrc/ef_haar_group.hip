// cv::groupRectangles(rects, minNeighbors, eps = 0.2) on the GPU: the last step of
// detectMultiScale (detection-v4.py:50-55, useless/scan.py:184-189), which ef_haar_detect runs
// on the host after copying every candidate back.  Here the candidates stay on the card, so
// ef_haar_scan_frame can hand the grouped rectangles straight to the ROI resize and the bank.
//
// The result equals ef_haar.hip's group_rectangles on the candidates sorted by (layer, y, x):
//   * SimilarRects is symmetric, so cv::partition's classes are the connected components of
//     the similarity graph, and it numbers them by their first member in list order.  A
//     component is therefore named by its member of smallest key (key = (layer, y, x) packed,
//     or the list index), and only the components are ordered, by that key: no sort of the
//     rectangles.
//   * Per class the sums of x, y, w, h and the member count are integers, so any order of
//     adding gives the host's values; the average is lrint((float)sum * (1.f / count)) in
//     the host's float operations.
//   * The neighbour threshold and the nested-rectangle rule look at one pair of classes at a
//     time; survivors keep the class order.
// Six launches, each a grid over the capacity maxc whose workgroups leave at once past the
// count read from device memory (no host read sizes anything):
//   init      candidate -> rectangle and key; every rectangle its own parent
//   union     all pairs i < j (256 x 256 tiles, the j tile in LDS): similar pairs are joined in
//             a lock-free union-find whose links always point to a smaller key
//   flatten   root[i] = the end of i's chain
//   classes   a thread per root walks every rectangle (tiles in LDS): sums and count of its
//             members, and its rank among the roots by key = its class index
//   filter    a thread per class walks every class: keep or drop
//   emit      a thread per class counts the kept classes before it and stores its rectangle
// Termination: the forest is acyclic by construction (a link goes to a smaller key), so a
// chain has at most n - 1 links; every chain walk is cut at n steps and every union at 2 n + 2
// attempts (a failed compare-and-swap means another thread linked that root, and the next
// attempt starts from strictly smaller roots).  A walk that reaches its bound sets
// EF_HAAR_SCAN_UNCONVERGED and gives up; nothing waits for another workgroup.
#include <algorithm>
#include <cstdint>
#include <cstring>
#include <string>
#include <vector>

#include "ef_haar.hpp"
#include "ef_union_find.hpp"

namespace ef {

namespace {

typedef unsigned long long u64;

__device__ __forceinline__ int group_count(const int* ncount, int maxc) {
  const int n = *ncount;
  return (n < 0 || n > maxc) ? 0 : n;
}

__global__ __launch_bounds__(256) void haar_group_init_kernel(const HaarCand* __restrict__ cand,
                                                              const HaarLayer* __restrict__ L, int ww, int wh,
                                                              const int* __restrict__ ncount, int n_host, int maxc,
                                                              HaarGroupWs ws, int* __restrict__ rects_out,
                                                              int max_rects) {
  const int gid = blockIdx.x * 256 + threadIdx.x;
  if (gid == 0) {
    ws.count[0] = 0;
    ws.count[1] = 0;
    if (!cand) ws.count[2] = n_host;
  }
  for (int64_t k = gid; k < (int64_t)max_rects * 4; k += (int64_t)gridDim.x * 256) rects_out[k] = 0;
  int n = cand ? *ncount : n_host;
  if (n < 0 || n > maxc) n = 0;
  if (gid >= n) return;
  if (cand) {
    // ef_haar_detect's arithmetic: a float product rounded half to even; w, h = cvRound(ww * sc)
    const HaarCand q = cand[gid];
    const float sc = L[q.layer].scale;
    ws.rect[gid] = make_int4(__float2int_rn(__fmul_rn((float)q.x, sc)), __float2int_rn(__fmul_rn((float)q.y, sc)),
                             __float2int_rn(__fmul_rn((float)ww, sc)), __float2int_rn(__fmul_rn((float)wh, sc)));
    ws.key[gid] = ((u64)(unsigned)q.layer << 48) | ((u64)((unsigned)q.y & 0xffffffu) << 24) | ((unsigned)q.x & 0xffffffu);
  } else {
    ws.key[gid] = (u64)gid;
  }
  ws.parent[gid] = gid;
}

// SimilarRects(eps = 0.2): delta in double as the host computes it
__device__ __forceinline__ bool similar_rects(const int4 a, const int4 b) {
  const double delta = __dmul_rn(__dmul_rn(0.2, (double)(min(a.z, b.z) + min(a.w, b.w))), 0.5);
  return (double)abs(a.x - b.x) <= delta && (double)abs(a.y - b.y) <= delta &&
         (double)abs(a.x + a.z - b.x - b.z) <= delta && (double)abs(a.y + a.w - b.y - b.w) <= delta;
}

__global__ __launch_bounds__(256) void haar_group_union_kernel(const int* __restrict__ ncount, int maxc, HaarGroupWs ws) {
  __shared__ int4 sr[256];
  const int n = group_count(ncount, maxc);
  const int i0 = blockIdx.x * 256, j0 = blockIdx.y * 256;
  if (blockIdx.y < blockIdx.x || j0 >= n) return;  // uniform; i0 <= j0 < n
  const int t = threadIdx.x;
  if (j0 + t < n) sr[t] = ws.rect[j0 + t];
  __syncthreads();
  const int i = i0 + t;
  if (i >= n) return;
  const int4 ri = ws.rect[i];
  const int m = min(256, n - j0);
  for (int jj = 0; jj < m; ++jj) {
    const int j = j0 + jj;
    if (j <= i || !similar_rects(ri, sr[jj])) continue;
    const u64* const key = ws.key;
    if (!group_union(ws.parent, i, j, n, [key](int a, int b) { return key[a] < key[b]; }))
      atomicOr(ws.count + 1, EF_HAAR_SCAN_UNCONVERGED);
  }
}

__global__ __launch_bounds__(256) void haar_group_flatten_kernel(const int* __restrict__ ncount, int maxc, HaarGroupWs ws) {
  const int n = group_count(ncount, maxc);
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  int r = group_find<false>(ws.parent, i, n);
  if (r < 0) {
    atomicOr(ws.count + 1, EF_HAAR_SCAN_UNCONVERGED);
    r = i;
  }
  ws.root[i] = r;
}

__global__ __launch_bounds__(256) void haar_group_classes_kernel(const int* __restrict__ ncount, int maxc, HaarGroupWs ws) {
  __shared__ int4 sr[256];
  __shared__ int sroot[256];
  __shared__ u64 skey[256];
  const int n = group_count(ncount, maxc);
  if (blockIdx.x * 256 >= n) return;  // uniform
  const int t = threadIdx.x, i = blockIdx.x * 256 + t;
  const bool is_root = i < n && ws.root[i] == i;
  const u64 ki = is_root ? ws.key[i] : 0;
  long long sx = 0, sy = 0, sw = 0, sh = 0;
  int cnt = 0, rank = 0, total = 0;
  for (int j0 = 0; j0 < n; j0 += 256) {
    if (j0 + t < n) {
      sr[t] = ws.rect[j0 + t];
      sroot[t] = ws.root[j0 + t];
      skey[t] = ws.key[j0 + t];
    }
    __syncthreads();
    if (is_root) {
      const int m = min(256, n - j0);
      for (int jj = 0; jj < m; ++jj) {
        const int rj = sroot[jj];
        if (rj == i) {
          const int4 r = sr[jj];
          sx += r.x, sy += r.y, sw += r.z, sh += r.w;
          ++cnt;
        }
        if (rj == j0 + jj) {
          ++total;
          rank += skey[jj] < ki;
        }
      }
    }
    __syncthreads();
  }
  if (!is_root) return;
  const float s = __fdiv_rn(1.f, (float)cnt);
  ws.cls_rect[rank] = make_int4(__float2int_rn(__fmul_rn(__ll2float_rn(sx), s)), __float2int_rn(__fmul_rn(__ll2float_rn(sy), s)),
                                __float2int_rn(__fmul_rn(__ll2float_rn(sw), s)), __float2int_rn(__fmul_rn(__ll2float_rn(sh), s)));
  ws.cls_cnt[rank] = cnt;
  if (rank == 0) ws.count[0] = total;
}

__global__ __launch_bounds__(256) void haar_group_filter_kernel(int maxc, int thr, HaarGroupWs ws) {
  __shared__ int4 sr[256];
  __shared__ int sc[256];
  const int nc = min(ws.count[0], maxc);
  if (blockIdx.x * 256 >= nc) return;  // uniform
  const int t = threadIdx.x, i = blockIdx.x * 256 + t;
  const int4 r1 = i < nc ? ws.cls_rect[i] : make_int4(0, 0, 0, 0);
  const int n1 = i < nc ? ws.cls_cnt[i] : 0;
  bool alive = i < nc && n1 > thr;
  for (int j0 = 0; j0 < nc; j0 += 256) {
    if (j0 + t < nc) {
      sr[t] = ws.cls_rect[j0 + t];
      sc[t] = ws.cls_cnt[j0 + t];
    }
    __syncthreads();
    const int m = min(256, nc - j0);
    for (int jj = 0; jj < m && alive; ++jj) {
      const int n2 = sc[jj];
      if (j0 + jj == i || n2 <= thr) continue;
      const int4 r2 = sr[jj];
      const int dx = __double2int_rn(__dmul_rn((double)r2.z, 0.2)), dy = __double2int_rn(__dmul_rn((double)r2.w, 0.2));
      if (r1.x >= r2.x - dx && r1.y >= r2.y - dy && r1.x + r1.z <= r2.x + r2.z + dx && r1.y + r1.w <= r2.y + r2.w + dy &&
          (n2 > max(3, n1) || n1 < 3))
        alive = false;
    }
    __syncthreads();
  }
  if (i < nc) ws.keep[i] = alive ? 1 : 0;
}

__global__ __launch_bounds__(256) void haar_group_emit_kernel(const int* __restrict__ ncount, int maxc, HaarGroupWs ws,
                                                              ef_haar_scan_head* __restrict__ head,
                                                              int* __restrict__ n_rects_out, int* __restrict__ rects_out,
                                                              int max_rects) {
  __shared__ int sk[256];
  const int nc = min(ws.count[0], maxc);
  const int nraw = *ncount;
  const int status = ws.count[1] | ((nraw < 0 || nraw > maxc) ? EF_HAAR_SCAN_OVERFLOW : 0);
  if (nc == 0) {
    if (blockIdx.x == 0 && threadIdx.x == 0) {
      if (head) *head = ef_haar_scan_head{status, nraw, 0, 0};
      if (n_rects_out) *n_rects_out = 0;
    }
    return;
  }
  if (blockIdx.x * 256 >= nc) return;  // uniform
  const int t = threadIdx.x, i = blockIdx.x * 256 + t;
  int pos = 0;
  for (int j0 = 0; j0 <= blockIdx.x * 256; j0 += 256) {  // the tiles that hold classes before this block's last
    if (j0 + t < nc) sk[t] = ws.keep[j0 + t];
    __syncthreads();
    const int m = min(256, min(nc, i) - j0);
    for (int jj = 0; jj < m; ++jj) pos += sk[jj];
    __syncthreads();
  }
  if (i >= nc) return;
  const int k = ws.keep[i];
  if (k && pos < max_rects) {
    const int4 r = ws.cls_rect[i];
    rects_out[4 * pos] = r.x, rects_out[4 * pos + 1] = r.y, rects_out[4 * pos + 2] = r.z, rects_out[4 * pos + 3] = r.w;
  }
  if (i == nc - 1) {
    const int total = pos + k;
    if (head) *head = ef_haar_scan_head{status, nraw, total, min(total, max_rects)};
    if (n_rects_out) *n_rects_out = total;
  }
}

}  // namespace

hipError_t launch_haar_group(hipStream_t s, const HaarCand* cand, const HaarLayer* layers, int ww, int wh,
                             const int* ncount, int n_host, int maxc, int min_neighbors, const HaarGroupWs& ws,
                             ef_haar_scan_head* head, int* n_rects_out, int* rects_out, int max_rects) {
  const unsigned tiles = (unsigned)((maxc + 255) / 256);
  if (!cand) ncount = ws.count + 2;  // written by the init kernel
  hipLaunchKernelGGL(haar_group_init_kernel, dim3(tiles), dim3(256), 0, s, cand, layers, ww, wh, ncount, n_host, maxc, ws,
                     rects_out, max_rects);
  hipLaunchKernelGGL(haar_group_union_kernel, dim3(tiles, tiles), dim3(256), 0, s, ncount, maxc, ws);
  hipLaunchKernelGGL(haar_group_flatten_kernel, dim3(tiles), dim3(256), 0, s, ncount, maxc, ws);
  hipLaunchKernelGGL(haar_group_classes_kernel, dim3(tiles), dim3(256), 0, s, ncount, maxc, ws);
  hipLaunchKernelGGL(haar_group_filter_kernel, dim3(tiles), dim3(256), 0, s, maxc, min_neighbors, ws);
  hipLaunchKernelGGL(haar_group_emit_kernel, dim3(tiles), dim3(256), 0, s, ncount, maxc, ws, head, n_rects_out, rects_out,
                     max_rects);
  return hipGetLastError();
}

}  // namespace ef

using namespace ef;

extern "C" int ef_haar_group(ef_ctx* c, const int32_t* rects, int32_t n, int32_t min_neighbors, int32_t* rects_out,
                             int32_t max_rects, int32_t* n_rects, uint32_t flags) {
  if (!c) return EF_E_INVALID;
  if (n < 0 || min_neighbors <= 0 || max_rects < 0 || !n_rects || (n > 0 && !rects) || (max_rects > 0 && !rects_out))
    return set_err(c, EF_E_INVALID, "ef_haar_group: bad arguments (min_neighbors must be >= 1)");
  EF_HIP(c, hipSetDevice(c->device), "hipSetDevice");
  hipStream_t s = c->stream;
  const bool dev = flags & EF_MEM_DEVICE;
  const int maxc = kHaarGroupMax;
  const int nin = std::min<int>(n, maxc);               // rectangles that fit the scratch
  const int nout = dev ? 0 : std::min<int>(max_rects, maxc);  // a host call's staged results
  Carve size, cv;
  carve_haar_group_ws(size, (size_t)maxc);
  size.take<ef_haar_scan_head>(1);
  size.take<int>((size_t)nout * 4 + 4);
  EF_TRY(ensure(c, c->haar_group_ws, size.total));
  cv.base = c->haar_group_ws.p;
  const HaarGroupWs ws = carve_haar_group_ws(cv, (size_t)maxc);
  ef_haar_scan_head* head = cv.take<ef_haar_scan_head>(1);
  int* stage = cv.take<int>((size_t)nout * 4 + 4);
  if (nin > 0)
    EF_HIP(c, hipMemcpyAsync(ws.rect, rects, (size_t)nin * 16, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, s),
           "rectangles");
  EF_HIP(c, launch_haar_group(s, nullptr, nullptr, 0, 0, nullptr, n, maxc, min_neighbors, ws, head, dev ? n_rects : nullptr,
                              dev ? rects_out : stage, dev ? max_rects : nout),
         "grouping kernels");
  const std::string over = "ef_haar_group: EF_HAAR_SCAN_OVERFLOW: more than " + std::to_string(maxc) + " rectangles";
  if (dev) return n > maxc ? set_err(c, EF_E_INVALID, over) : EF_OK;
  // head and the staged rectangles are neighbours in the scratch: one download
  const size_t bytes = (size_t)(reinterpret_cast<char*>(stage) - reinterpret_cast<char*>(head)) + (size_t)nout * 16;
  std::vector<char> host(bytes);
  EF_HIP(c, hipMemcpyAsync(host.data(), head, bytes, hipMemcpyDeviceToHost, s), "D2H grouped rectangles");
  EF_HIP(c, hipStreamSynchronize(s), "sync");
  const ef_haar_scan_head* hh = reinterpret_cast<const ef_haar_scan_head*>(host.data());
  *n_rects = hh->n_rects;
  if (hh->status & EF_HAAR_SCAN_OVERFLOW) return set_err(c, EF_E_INVALID, over);
  if (hh->status & EF_HAAR_SCAN_UNCONVERGED)
    return set_err(c, EF_E_NUMERIC, "ef_haar_group: a grouping loop reached its iteration bound");
  const int got = std::min<int>(hh->n_rects, nout);
  if (got > 0) std::memcpy(rects_out, host.data() + (bytes - (size_t)nout * 16), (size_t)got * 16);
  return EF_OK;
}
