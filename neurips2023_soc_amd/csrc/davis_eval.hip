// K27: the per-pixel part of the DAVIS J&F evaluation (davis2017/metrics.py:6-37 db_eval_iou, :57-119 f_measure,
// :122-178 _seg2bmap; the loops of davis2017/evaluation.py:28-64 over objects, proposals and frames), on label maps that
// are already on the device.  Everything the reference computes per (ground-truth object i, predicted object j, frame t)
// is a function of six integers,
//     inter = sum(fg & gt & ~void)      union    = sum((fg | gt) & ~void)
//     n_fg  = sum(fb)                   n_gt     = sum(gb)                 fb / gb = seg2bmap(fg / gt & ~void)
//     fg_match = sum(fb & dil(gb))      gt_match = sum(gb & dil(fb))       dil = dilation by the disk of `radius`
// and this file produces exactly those; the few f64 operations on them stay on the host (davis_eval.jf_from_counts), in
// the reference's order, so the result is exact and bit-repeatable (integer sums commute).
//
// Layout: one bit per pixel.  A plane is H rows of WPR = ceil(W / 64) 64-bit words, bit b of word wx = pixel x = 64 wx + b
// (a wave's __ballot over 64 neighbouring pixels is one word); the bits of a row's last word beyond W are zero in every
// plane, always.  Per frame there are NP = G + P planes (objects 1..G of the ground truth, then 1..P of the prediction) in
// three sets: mask, boundary, dilated boundary.  Four kernels, in stream order, per chunk of frames that fits the workspace:
//   planes    label maps -> mask planes                 one wave per (frame, row, word): one read of the label maps
//   boundary  mask -> boundary planes                   _seg2bmap on bit rows: shifts and XORs, then the last-row /
//                                                       last-column / corner rules
//   dilate    boundary -> dilated planes                each plane once; a workgroup stages a 32-row x 32-word tile plus
//                                                       `radius` halo rows and one halo word per side in LDS (<= 43.5 KB at
//                                                       radius 64); rows / words outside the image are zero there
//   counts    AND / OR + popcount over planes           one workgroup per (pair, frame), written straight into `counts`
//
// K27b (soc_hip_jf_bits.h), the per-expression form: E predictions that are ALREADY bit planes in this layout (K6b's output,
// packed_masks.py) against O distinct ground-truth objects, expression e against object exp_obj[e].  Per frame there are
// NP = O + E planes (objects, then expressions); the planes kernel builds the O object planes from the label maps with
// ballots, as above, and the E prediction planes by one 64-bit load per word, ANDed with the wave's "inside the image and
// not void" ballot -- the predictions are never expanded to bytes, and their padding bits never reach a plane.  Boundary
// and dilation are the kernels above, run once per plane: an object's three planes serve every expression that names it.
#include "soc_common.h"
#include "soc_hip_jf_bits.h"

namespace {

typedef unsigned long long u64;

constexpr int MAX_RADIUS = 64;
constexpr int DIL_BH = 32;          // rows of a dilation tile
constexpr int DIL_WT = 32;          // words of a dilation tile
constexpr size_t CHUNK_BYTES = (size_t)64 << 20;   // frames are processed in chunks whose planes fit this

struct DiskTable { uint8_t w[MAX_RADIUS + 1]; };   // w[|dy|] = floor(sqrt(r^2 - dy^2)), integer arithmetic on the host

__global__ __launch_bounds__(256) void planes_kernel(const uint8_t* __restrict__ gt, const uint8_t* __restrict__ pred,
                                                     u64* __restrict__ mask, int G, int P, int H, int W, int WPR,
                                                     int use_void, long n_words) {
    const int lane = threadIdx.x & 63;
    const long word = (long)blockIdx.x * 4 + (threadIdx.x >> 6);      // (frame, row, word) of this wave
    if (word >= n_words) return;                                       // whole waves leave: the ballots below stay full
    const int wx = (int)(word % WPR);
    const long fy = word / WPR;                                        // frame * H + y
    const int y = (int)(fy % H);
    const long f = fy / H;
    const int x = wx * 64 + lane;
    int g = 0, p = 0;
    if (x < W) {
        g = gt[fy * W + x];
        p = pred[fy * W + x];
        if (use_void && g == 255) g = p = -1;                          // a void pixel belongs to no plane
    } else {
        g = p = -1;
    }
    const int NP = G + P;
    for (int base = 0; base < NP; base += 64) {
        const int n = NP - base < 64 ? NP - base : 64;
        u64 mine = 0;
        for (int k = 0; k < n; ++k) {
            const int pl = base + k;
            const bool on = pl < G ? (g == pl + 1) : (p == pl - G + 1);
            const u64 b = __ballot(on);
            if (lane == k) mine = b;
        }
        if (lane < n) mask[((f * NP + base + lane) * H + y) * WPR + wx] = mine;
    }
}

// _seg2bmap (metrics.py:154-165): e / s / se are the mask shifted by one towards the origin (zero filled),
// b = seg^e | seg^s | seg^se, then the last row is seg^e, the last column seg^s, the corner 0 -- in that order.
__global__ __launch_bounds__(256) void boundary_kernel(const u64* __restrict__ mask, u64* __restrict__ bnd, int H, int W,
                                                       int WPR, long n_words) {
    const long word = (long)blockIdx.x * 256 + threadIdx.x;           // (plane, row, word)
    if (word >= n_words) return;
    const int wx = (int)(word % WPR);
    const int y = (int)((word / WPR) % H);
    const bool last_row = y == H - 1, last_word = wx == WPR - 1;
    const u64 seg = mask[word];
    const u64 segn = last_word ? 0 : mask[word + 1];
    const u64 s = last_row ? 0 : mask[word + WPR];
    const u64 sn = (last_row || last_word) ? 0 : mask[word + WPR + 1];
    const u64 e = (seg >> 1) | (segn << 63);                           // e[x] = seg[x + 1]; zero at x = W - 1 (tail bits are zero)
    const u64 se = (s >> 1) | (sn << 63);
    u64 b = last_row ? (seg ^ e) : ((seg ^ e) | (seg ^ s) | (seg ^ se));
    if (last_word) {
        const u64 col = 1ull << ((W - 1) & 63);
        b = (b & ~col) | (last_row ? 0 : ((seg ^ s) & col));
    }
    bnd[word] = b;
}

// OR of the row shifted by -w .. w pixels, for the middle word of (lo, mid, hi): shift-OR doubling on the 128-bit pairs
// (lo, mid) upwards and (mid, hi) downwards; w <= 64, so no word further away can reach `mid`.
__device__ inline u64 hdil(u64 lo, u64 mid, u64 hi, int w) {
    u64 up = mid, dn = mid;
    for (int cov = 0; cov < w;) {
        const int s = cov + 1 < w - cov ? cov + 1 : w - cov;           // 1 <= s <= 32
        up |= (up << s) | (lo >> (64 - s));
        lo |= lo << s;
        dn |= (dn >> s) | (hi << (64 - s));
        hi |= hi >> s;
        cov += s;
    }
    return up | dn;
}

// cv2.dilate(b, skimage.morphology.disk(r)) on a binary image (metrics.py:84-89): (y, x) is set iff some (dy, dx) with
// dx^2 + dy^2 <= r^2 has (y + dy, x + dx) inside the image and set, i.e. OR over dy of hdil(row y + dy, w(dy)).
__global__ __launch_bounds__(256) void dilate_kernel(const u64* __restrict__ bnd, u64* __restrict__ dil, int H, int W,
                                                     int WPR, int r, DiskTable tab, int tiles_x, int tiles_y) {
    extern __shared__ u64 tile[];
    long b = blockIdx.x;
    const int tx = (int)(b % tiles_x); b /= tiles_x;
    const int ty = (int)(b % tiles_y);
    const long plane = b / tiles_y;
    const int wt = WPR < DIL_WT ? WPR : DIL_WT;
    const int lw = wt + 2, rows = DIL_BH + 2 * r;
    const int y0 = ty * DIL_BH - r, x0 = tx * wt - 1;
    const u64* src = bnd + plane * H * WPR;
    for (int i = threadIdx.x; i < rows * lw; i += 256) {
        const int y = y0 + i / lw, x = x0 + i % lw;
        tile[i] = (y >= 0 && y < H && x >= 0 && x < WPR) ? src[(long)y * WPR + x] : 0;
    }
    __syncthreads();
    u64* dst = dil + plane * H * WPR;
    for (int i = threadIdx.x; i < DIL_BH * wt; i += 256) {
        const int oy = i / wt, ox = i % wt;
        const int y = ty * DIL_BH + oy, x = tx * wt + ox;
        if (y >= H || x >= WPR) continue;
        u64 acc = 0;
        for (int dy = -r; dy <= r; ++dy) {
            const u64* row = tile + (oy + r + dy) * lw + ox;           // row[0..2]: the words x - 1, x, x + 1 of row y + dy
            const u64 lo = row[0], mid = row[1], hi = row[2];
            if (lo | mid | hi) acc |= hdil(lo, mid, hi, tab.w[dy < 0 ? -dy : dy]);
        }
        if (x == WPR - 1 && (W & 63)) acc &= (1ull << (W & 63)) - 1;   // nothing is set beyond the image
        dst[(long)y * WPR + x] = acc;
    }
}

// The six counts of ground-truth plane `gi` against prediction plane `pj` (word offsets of the planes; no prediction: an
// empty mask), summed by the whole workgroup and written to out[0..5].
__device__ inline void count_planes(const u64* __restrict__ mask, const u64* __restrict__ bnd, const u64* __restrict__ dil,
                                    long gi, long pj, bool have_pred, long plane_words, int32_t* __restrict__ out) {
    __shared__ int acc[6];
    if (threadIdx.x < 6) acc[threadIdx.x] = 0;
    __syncthreads();
    int c[6] = {0, 0, 0, 0, 0, 0};
    for (long k = threadIdx.x; k < plane_words; k += 256) {
        const u64 gm = mask[gi + k], gb = bnd[gi + k], gd = dil[gi + k];
        const u64 pm = have_pred ? mask[pj + k] : 0, pb = have_pred ? bnd[pj + k] : 0, pd = have_pred ? dil[pj + k] : 0;
        c[0] += __popcll(pm & gm);
        c[1] += __popcll(pm | gm);
        c[2] += __popcll(pb);
        c[3] += __popcll(gb);
        c[4] += __popcll(pb & gd);
        c[5] += __popcll(gb & pd);
    }
#pragma unroll
    for (int q = 0; q < 6; ++q) {
        int v = c[q];
        for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
        if ((threadIdx.x & 63) == 0) atomicAdd(&acc[q], v);            // integer: the order does not matter
    }
    __syncthreads();
    if (threadIdx.x < 6) out[threadIdx.x] = acc[threadIdx.x];
}

// One workgroup per (row of `counts`, frame of the chunk).  pairs: row = i * P + j; otherwise row = k (object k against
// prediction k, an empty mask for k >= P).
__global__ __launch_bounds__(256) void counts_kernel(const u64* __restrict__ mask, const u64* __restrict__ bnd,
                                                     const u64* __restrict__ dil, int32_t* __restrict__ counts, int G, int P,
                                                     int T, int t0, int Tc, long plane_words, int pairs) {
    const int tl = blockIdx.x % Tc;
    const int row = blockIdx.x / Tc;
    const int i = pairs ? row / P : row;
    const int j = pairs ? row % P : row;
    const bool have_pred = j < P;
    const int NP = G + P;
    const long gi = ((long)tl * NP + i) * plane_words;
    const long pj = ((long)tl * NP + G + (have_pred ? j : 0)) * plane_words;
    count_planes(mask, bnd, dil, gi, pj, have_pred, plane_words, counts + ((long)row * T + t0 + tl) * 6);
}

// K27b ------------------------------------------------------------------------------------------------------------------
// The two id lists travel by value in the kernel arguments: nothing is allocated, copied or remembered for them.
struct IdTable {
    uint8_t obj[SOC_JF_BITS_MAX];      // label of object k, 1..254
    uint8_t exp[SOC_JF_BITS_MAX];      // object index of expression e
};

// One wave per (frame, row, word) of the chunk.  `pred` points at the chunk's first frame of expression 0; expression e is
// exp_stride BYTES further on; both are multiples of 8, so every word is one aligned 64-bit load.
__global__ __launch_bounds__(256) void planes_bits_kernel(const uint8_t* __restrict__ gt, const uint8_t* __restrict__ pred,
                                                          long exp_stride, u64* __restrict__ mask, IdTable ids, int O, int E,
                                                          int H, int W, int WPR, int use_void, long n_words) {
    const int lane = threadIdx.x & 63;
    const long word = (long)blockIdx.x * 4 + (threadIdx.x >> 6);      // (frame, row, word) of this wave
    if (word >= n_words) return;                                       // whole waves leave: the ballots below stay full
    const int wx = (int)(word % WPR);
    const long fy = word / WPR;                                        // frame * H + y
    const int y = (int)(fy % H);
    const long f = fy / H;
    const int x = wx * 64 + lane;
    int g = -1;                                                        // outside the image or void: in no plane
    if (x < W) {
        g = gt[fy * W + x];
        if (use_void && g == 255) g = -1;
    }
    const u64 keep = __ballot(g >= 0);
    const int NP = O + E;
    for (int base = 0; base < O; base += 64) {
        const int n = O - base < 64 ? O - base : 64;
        u64 mine = 0;
        for (int k = 0; k < n; ++k) {
            const u64 b = __ballot(g == (int)ids.obj[base + k]);
            if (lane == k) mine = b;
        }
        if (lane < n) mask[((f * NP + base + lane) * H + y) * WPR + wx] = mine;
    }
    for (int e = lane; e < E; e += 64) {                               // lane e: the word of expression e
        const u64 p = *(const u64*)(pred + (size_t)e * exp_stride + (size_t)word * sizeof(u64));
        mask[((f * NP + O + e) * H + y) * WPR + wx] = p & keep;
    }
}

// One workgroup per (expression, frame of the chunk).
__global__ __launch_bounds__(256) void counts_bits_kernel(const u64* __restrict__ mask, const u64* __restrict__ bnd,
                                                          const u64* __restrict__ dil, int32_t* __restrict__ counts,
                                                          IdTable ids, int O, int E, int T, int t0, int Tc, long plane_words) {
    const int tl = blockIdx.x % Tc;
    const int e = blockIdx.x / Tc;
    const int NP = O + E;
    const long gi = ((long)tl * NP + ids.exp[e]) * plane_words;
    const long pj = ((long)tl * NP + O + e) * plane_words;
    count_planes(mask, bnd, dil, gi, pj, true, plane_words, counts + ((long)e * T + t0 + tl) * 6);
}

inline size_t frame_bytes(int G, int P, int H, int W) {
    return (size_t)(G + P) * (size_t)H * (size_t)soc_ceil_div(W, 64) * sizeof(u64) * 3;
}

inline int chunk_frames(int G, int P, int T, int H, int W) {
    const size_t per = frame_bytes(G, P, H, W);
    size_t n = per ? CHUNK_BYTES / per : (size_t)T;
    if (n < 1) n = 1;
    return n < (size_t)T ? (int)n : T;
}

inline bool sizes_ok(int G, int P, int T, int H, int W) {
    return G >= 0 && G <= 255 && P >= 0 && P <= 255 && G + P > 0 && T > 0 && H > 0 && W > 0;
}

inline DiskTable disk_table(int radius) {
    DiskTable tab;
    for (int dy = 0; dy <= MAX_RADIUS; ++dy) {
        int w = 0;
        if (dy <= radius)
            while ((w + 1) * (w + 1) + dy * dy <= radius * radius) ++w;
        tab.w[dy] = (uint8_t)w;
    }
    return tab;
}

inline bool bits_sizes_ok(int E, int O, int H, int W) {
    return E >= 1 && E <= SOC_JF_BITS_MAX && O >= 1 && O <= SOC_JF_BITS_MAX && H > 0 && W > 0 && (long)H * W <= 0x7fffffffL;
}

}  // namespace

extern "C" size_t soc_davis_jf_workspace_bytes(int G, int P, int T, int H, int W) {
    if (!sizes_ok(G, P, T, H, W)) return 0;
    return (size_t)chunk_frames(G, P, T, H, W) * frame_bytes(G, P, H, W);
}

extern "C" int soc_davis_jf_counts_u8(const uint8_t* gt_labels, const uint8_t* pred_labels, int32_t* counts, int G, int P,
                                      int T, int H, int W, int radius, int use_void, int pairs, void* workspace,
                                      size_t workspace_bytes, void* stream) {
    if (!gt_labels || !pred_labels || !counts || !workspace || T <= 0 || H <= 0 || W <= 0) return SOC_EINVAL;
    if (radius < 0 || radius > MAX_RADIUS || !sizes_ok(G, P, T, H, W)) return SOC_EUNSUPPORTED;
    if ((long)H * W > 0x7fffffffL) return SOC_EUNSUPPORTED;            // the counts are 32-bit
    if (workspace_bytes < soc_davis_jf_workspace_bytes(G, P, T, H, W)) return SOC_EWORKSPACE;
    const int n_rows = pairs ? G * P : G;
    if (n_rows == 0) return SOC_OK;                                    // an empty `counts`
    const DiskTable tab = disk_table(radius);
    const int NP = G + P, WPR = soc_ceil_div(W, 64);
    const long plane_words = (long)H * WPR;
    const int Tc = chunk_frames(G, P, T, H, W);
    const int wt = WPR < DIL_WT ? WPR : DIL_WT;
    const int tiles_x = soc_ceil_div(WPR, wt), tiles_y = soc_ceil_div(H, DIL_BH);
    const size_t lds = (size_t)(DIL_BH + 2 * radius) * (wt + 2) * sizeof(u64);
    hipStream_t st = (hipStream_t)stream;
    for (int t0 = 0; t0 < T; t0 += Tc) {
        const int tc = T - t0 < Tc ? T - t0 : Tc;
        u64* mask = (u64*)workspace;
        u64* bnd = mask + (size_t)tc * NP * plane_words;
        u64* dil = bnd + (size_t)tc * NP * plane_words;
        const long px_words = (long)tc * plane_words, all_words = px_words * NP;
        hipLaunchKernelGGL(planes_kernel, dim3(soc_ceil_div(px_words, 4)), dim3(256), 0, st, gt_labels + (size_t)t0 * H * W,
                           pred_labels + (size_t)t0 * H * W, mask, G, P, H, W, WPR, use_void, px_words);
        hipLaunchKernelGGL(boundary_kernel, dim3(soc_ceil_div(all_words, 256)), dim3(256), 0, st, mask, bnd, H, W, WPR,
                           all_words);
        hipLaunchKernelGGL(dilate_kernel, dim3((unsigned)((long)tc * NP * tiles_y * tiles_x)), dim3(256), lds, st, bnd, dil,
                           H, W, WPR, radius, tab, tiles_x, tiles_y);
        hipLaunchKernelGGL(counts_kernel, dim3((unsigned)((long)n_rows * tc)), dim3(256), 0, st, mask, bnd, dil, counts, G, P,
                           T, t0, tc, plane_words, pairs);
        const int code = soc_check_launch();
        if (code != SOC_OK) return code;
    }
    return SOC_OK;
}

extern "C" size_t soc_jf_bits_workspace_bytes(int E, int O, int H, int W) {
    return bits_sizes_ok(E, O, H, W) ? frame_bytes(O, E, H, W) : 0;
}

extern "C" int soc_jf_counts_bits(const uint8_t* gt_labels, const uint8_t* pred_bits, long exp_stride, const int* obj_ids,
                                  const int* exp_obj, int32_t* counts, int E, int O, int T, int H, int W, int radius,
                                  int use_void, void* workspace, size_t workspace_bytes, void* stream) {
    if (!gt_labels || !pred_bits || !obj_ids || !exp_obj || !counts || !workspace || E <= 0 || O <= 0 || T <= 0 || H <= 0 ||
        W <= 0)
        return SOC_EINVAL;
    if (((uintptr_t)pred_bits & 7) || (exp_stride & 7)) return SOC_EINVAL;       // the planes are read as 64-bit words
    if (radius < 0 || radius > MAX_RADIUS || !bits_sizes_ok(E, O, H, W)) return SOC_EUNSUPPORTED;
    const int WPR = soc_ceil_div(W, 64);
    const long plane_words = (long)H * WPR;
    if (exp_stride < (long)T * plane_words * (long)sizeof(u64)) return SOC_EUNSUPPORTED;
    IdTable ids = {};
    for (int k = 0; k < O; ++k) {
        if (obj_ids[k] < 1 || obj_ids[k] > 254) return SOC_EUNSUPPORTED;
        ids.obj[k] = (uint8_t)obj_ids[k];
    }
    for (int e = 0; e < E; ++e) {
        if (exp_obj[e] < 0 || exp_obj[e] >= O) return SOC_EUNSUPPORTED;
        ids.exp[e] = (uint8_t)exp_obj[e];
    }
    const size_t per = frame_bytes(O, E, H, W);
    if (workspace_bytes < per) return SOC_EWORKSPACE;
    // frames per chunk: what the workspace holds, at most CHUNK_BYTES of planes (more buys nothing and the grids stay small)
    size_t fit = (workspace_bytes < CHUNK_BYTES ? workspace_bytes : CHUNK_BYTES) / per;
    if (fit < 1) fit = 1;
    const int Tc = fit < (size_t)T ? (int)fit : T;
    const DiskTable tab = disk_table(radius);
    const int NP = O + E;
    const int wt = WPR < DIL_WT ? WPR : DIL_WT;
    const int tiles_x = soc_ceil_div(WPR, wt), tiles_y = soc_ceil_div(H, DIL_BH);
    const size_t lds = (size_t)(DIL_BH + 2 * radius) * (wt + 2) * sizeof(u64);
    hipStream_t st = (hipStream_t)stream;
    for (int t0 = 0; t0 < T; t0 += Tc) {
        const int tc = T - t0 < Tc ? T - t0 : Tc;
        u64* mask = (u64*)workspace;
        u64* bnd = mask + (size_t)tc * NP * plane_words;
        u64* dil = bnd + (size_t)tc * NP * plane_words;
        const long px_words = (long)tc * plane_words, all_words = px_words * NP;
        hipLaunchKernelGGL(planes_bits_kernel, dim3(soc_ceil_div(px_words, 4)), dim3(256), 0, st,
                           gt_labels + (size_t)t0 * H * W, pred_bits + (size_t)t0 * plane_words * sizeof(u64), exp_stride, mask,
                           ids, O, E, H, W, WPR, use_void, px_words);
        hipLaunchKernelGGL(boundary_kernel, dim3(soc_ceil_div(all_words, 256)), dim3(256), 0, st, mask, bnd, H, W, WPR,
                           all_words);
        hipLaunchKernelGGL(dilate_kernel, dim3((unsigned)((long)tc * NP * tiles_y * tiles_x)), dim3(256), lds, st, bnd, dil,
                           H, W, WPR, radius, tab, tiles_x, tiles_y);
        hipLaunchKernelGGL(counts_bits_kernel, dim3((unsigned)((long)E * tc)), dim3(256), 0, st, mask, bnd, dil, counts, ids, O,
                           E, T, t0, tc, plane_words);
        const int code = soc_check_launch();
        if (code != SOC_OK) return code;
    }
    return SOC_OK;
}
