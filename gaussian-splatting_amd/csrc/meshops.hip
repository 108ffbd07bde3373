// Mesh clean-up on an indexed triangle mesh (include/gsr.h): connected components over vertices, faces per component,
// compaction by a face mask, area-weighted vertex normals and Taubin smoothing -- what 2DGS's post_process_mesh and its kin do before a mesh is
// saved, here next to the extraction that made it.
//
// One rule for every kernel: row f of faces[nf,3] is a FACE iff its three indices are in [0, nv) and pairwise different (load_face).  Any other row is
// not there: nothing is read through it, it joins nothing, it counts nowhere and survives no compaction.
//
// Components: parent[v] = v (the caller's vertex_label IS the parent array), then rounds of hook + compress.  Hook: per face and edge, an integer
// atomicMin of the smaller of the two ends' current parents into the slot of the larger.  Compress: every vertex walks to its root (parent[p] < p off
// a root, so the walk ends) and points at it.  Labels only fall and stay inside the component, so at the fixpoint -- a round that hooked nothing: every
// tree flat, every edge with equal roots -- the label is the component's smallest vertex, whatever the schedule was.  The host reads one word per round.
// Per-vertex sums (normals, smoothing) run over the vertex's corners in ascending face order: the corners are sorted by vertex with sort.hip's stable
// LSD pair sort, every operand is converted to fp64 first and the unit is built with -ffp-contract=off, so the host build, the device and the numpy
// reference of tests/meshops_reference.py perform the same operations in the same order.  No floating-point atomics anywhere.
#include "gsr_internal.h"
#include "gsr_wave.h"

namespace {

constexpr int kBlock = 256;

struct Face { int a, b, c; bool ok; };

__device__ __forceinline__ Face load_face(const int32_t* __restrict__ faces, int64_t f, int nv) {
    Face t;
    t.a = faces[3 * f]; t.b = faces[3 * f + 1]; t.c = faces[3 * f + 2];
    t.ok = (uint32_t)t.a < (uint32_t)nv && (uint32_t)t.b < (uint32_t)nv && (uint32_t)t.c < (uint32_t)nv && t.a != t.b && t.b != t.c && t.a != t.c;
    return t;
}

struct MeshopsScratch {
    uint32_t* word;           // [32] word 0: the round that last hooked something
    uint32_t* mark;           // [nv] 1: a kept face uses the vertex
    uint32_t* remap;          // [nv] index of a kept vertex in the compacted mesh
    uint32_t* hist;           // [2][nb] kept vertices / kept faces per workgroup, then their exclusive prefixes
    int nb;
    uint32_t* keys[2];        // [3 nf] x2 corner sort: vertex id (nv for a corner of a row that is no face)
    uint32_t* vals[2];        // [3 nf] x2 corner index 3 f + k
    uint32_t* sort_hist;
    uint32_t* digit_total;    // [2048]
    uint32_t* start;          // [nv + 1] first sorted corner of every vertex; start[nv] = corners of faces
    float* tmp;               // [3 nv] the smoothing's second buffer
    size_t bytes;
};

inline int blocks_for(int64_t n) { return (int)((n + kBlock - 1) / kBlock); }
inline int sort_items(int64_t n3) { return n3 < (1 << 21) ? GSR_SORT_ITEMS_SMALL : GSR_SORT_ITEMS; }

inline MeshopsScratch carve(void* scratch, int nv, int nf) {
    MeshopsScratch m;
    size_t off = 0;      // (scratch == NULL: the size only)
    auto take = [&](size_t bytes) { char* q = scratch ? (char*)scratch + off : nullptr; off += gsr_align128(bytes); return q; };
    const int64_t n3 = 3 * (int64_t)nf;
    m.nb = blocks_for(nv > nf ? nv : nf);
    m.word = (uint32_t*)take(128);
    m.mark = (uint32_t*)take((size_t)nv * 4);
    m.remap = (uint32_t*)take((size_t)nv * 4);
    m.hist = (uint32_t*)take((size_t)2 * m.nb * 4);
    for (int i = 0; i < 2; ++i) m.keys[i] = (uint32_t*)take((size_t)n3 * 4);
    for (int i = 0; i < 2; ++i) m.vals[i] = (uint32_t*)take((size_t)n3 * 4);
    m.sort_hist = (uint32_t*)take((size_t)256 * (size_t)((n3 + sort_items(n3) - 1) / sort_items(n3)) * 4);
    m.digit_total = (uint32_t*)take(2048 * 4);
    m.start = (uint32_t*)take(((size_t)nv + 1) * 4);
    m.tmp = (float*)take((size_t)nv * 12);
    m.bytes = off;
    return m;
}

// ---- connected components -----------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
cc_init_kernel(int nv, int32_t* __restrict__ parent, int32_t* __restrict__ face_count, uint32_t* __restrict__ word) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v == 0) word[0] = 0u;
    if (v >= nv) return;
    parent[v] = (int32_t)v;
    face_count[v] = 0;
}

__device__ __forceinline__ bool hook(int32_t* parent, int u, int v) {
    const int ru = parent[u], rv = parent[v];      // (parent is written by this launch: no __restrict__, no cached copy)
    if (ru == rv) return false;
    atomicMin(&parent[ru > rv ? ru : rv], ru > rv ? rv : ru);
    return true;
}

__global__ void __launch_bounds__(kBlock)
cc_hook_kernel(int nv, int64_t nf, const int32_t* __restrict__ faces, int32_t* parent, uint32_t* __restrict__ word, uint32_t round) {
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (f >= nf) return;
    const Face t = load_face(faces, f, nv);
    if (!t.ok) return;
    const bool h0 = hook(parent, t.a, t.b), h1 = hook(parent, t.b, t.c), h2 = hook(parent, t.c, t.a);
    if (h0 | h1 | h2) word[0] = round;      // every writer of a round stores the same value
}

__global__ void __launch_bounds__(kBlock)
cc_compress_kernel(int nv, int32_t* parent) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    int p = parent[v];
    for (int q = parent[p]; q != p; q = parent[p]) p = q;      // strictly falling: ends at a root
    parent[v] = p;
}

// face_count[label] += faces with that label: one atomic per run of equal labels in the wave (a scene's main component holds nearly all faces, so
// whole waves are one run)
__global__ void __launch_bounds__(kBlock)
cc_face_count_kernel(int nv, int64_t nf, const int32_t* __restrict__ faces, const int32_t* __restrict__ label, int32_t* __restrict__ face_count) {
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63);
    int mine = -1;
    if (f < nf) {
        const Face t = load_face(faces, f, nv);
        if (t.ok) mine = label[t.a];
    }
    const int prev = __shfl_up(mine, 1);
    const uint64_t heads = __ballot(lane == 0 || prev != mine);
    if (mine < 0 || !((heads >> lane) & 1ull)) return;
    const uint64_t above = lane == 63 ? 0ull : heads >> (lane + 1);
    atomicAdd(&face_count[mine], above ? (int)__ffsll((unsigned long long)above) : 64 - lane);
}

// ---- compaction by a face mask ------------------------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
compact_clear_kernel(int nv, uint32_t* __restrict__ mark) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v < nv) mark[v] = 0u;
}

__device__ __forceinline__ bool kept_face(const Face& t, const uint8_t* __restrict__ keep, int64_t f) { return t.ok && (!keep || keep[f] != 0); }

__global__ void __launch_bounds__(kBlock)
compact_mark_kernel(int nv, int64_t nf, const int32_t* __restrict__ faces, const uint8_t* __restrict__ keep, uint32_t* __restrict__ mark) {
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (f >= nf) return;
    const Face t = load_face(faces, f, nv);
    if (!kept_face(t, keep, f)) return;
    mark[t.a] = 1u; mark[t.b] = 1u; mark[t.c] = 1u;      // (every writer stores the same value)
}

// workgroup b counts the kept vertices and the kept faces of its 256 of each
__global__ void __launch_bounds__(kBlock)
compact_count_kernel(int nv, int64_t nf, const int32_t* __restrict__ faces, const uint8_t* __restrict__ keep, MeshopsScratch m) {
    __shared__ uint32_t wsum[gsrw::WG_WAVES];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    uint32_t kv = 0, kf = 0;
    if (i < nv) kv = m.mark[i];
    if (i < nf) kf = kept_face(load_face(faces, i, nv), keep, i) ? 1u : 0u;
    const uint32_t v[1] = {kv | kf << 16};      // both counts through one scan: at most 256 each
    const uint32_t excl = gsrw::block_excl_scan<1>(v, wsum, (int)(threadIdx.x & 63), (int)(threadIdx.x >> 6));
    if (threadIdx.x == kBlock - 1) {
        const uint32_t total = excl + v[0];
        m.hist[blockIdx.x] = total & 0xFFFFu;
        m.hist[m.nb + blockIdx.x] = total >> 16;
    }
}

template <bool COLOR>
__global__ void __launch_bounds__(kBlock)
compact_emit_vertices_kernel(int nv, MeshopsScratch m, const float* __restrict__ vertices, const float* __restrict__ colors, int nv_out,
                             float* __restrict__ vertices_out, float* __restrict__ colors_out) {
    __shared__ uint32_t wsum[gsrw::WG_WAVES];
    const int64_t i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    const uint32_t v[1] = {i < nv ? m.mark[i] : 0u};
    const uint32_t excl = gsrw::block_excl_scan<1>(v, wsum, (int)(threadIdx.x & 63), (int)(threadIdx.x >> 6));
    if (!v[0]) return;
    const int64_t at = (int64_t)m.hist[blockIdx.x] + excl;
    m.remap[i] = (uint32_t)at;
    if (at >= nv_out) return;      // (a caller's nv_out below the count must not write past its buffer)
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        vertices_out[3 * at + k] = vertices[3 * i + k];
        if (COLOR) colors_out[3 * at + k] = colors[3 * i + k];
    }
}

__global__ void __launch_bounds__(kBlock)
compact_emit_faces_kernel(int nv, int64_t nf, MeshopsScratch m, const int32_t* __restrict__ faces, const uint8_t* __restrict__ keep, int nf_out,
                          int32_t* __restrict__ faces_out) {
    __shared__ uint32_t wsum[gsrw::WG_WAVES];
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    Face t;
    t.a = t.b = t.c = 0; t.ok = false;
    if (f < nf) t = load_face(faces, f, nv);
    const uint32_t v[1] = {f < nf && kept_face(t, keep, f) ? 1u : 0u};
    const uint32_t excl = gsrw::block_excl_scan<1>(v, wsum, (int)(threadIdx.x & 63), (int)(threadIdx.x >> 6));
    if (!v[0]) return;
    const int64_t at = (int64_t)m.hist[m.nb + blockIdx.x] + excl;
    if (at >= nf_out) return;
    faces_out[3 * at] = (int32_t)m.remap[t.a];
    faces_out[3 * at + 1] = (int32_t)m.remap[t.b];
    faces_out[3 * at + 2] = (int32_t)m.remap[t.c];
}

// ---- incident-face lists: corners sorted by vertex ----------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kBlock)
corner_keys_kernel(int nv, int64_t nf, const int32_t* __restrict__ faces, uint32_t* __restrict__ keys, uint32_t* __restrict__ vals) {
    const int64_t f = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (f >= nf) return;
    const Face t = load_face(faces, f, nv);
    keys[3 * f] = t.ok ? (uint32_t)t.a : (uint32_t)nv;
    keys[3 * f + 1] = t.ok ? (uint32_t)t.b : (uint32_t)nv;
    keys[3 * f + 2] = t.ok ? (uint32_t)t.c : (uint32_t)nv;
    vals[3 * f] = (uint32_t)(3 * f); vals[3 * f + 1] = (uint32_t)(3 * f + 1); vals[3 * f + 2] = (uint32_t)(3 * f + 2);
}

// start[v] = first sorted corner whose key is >= v, for v = 0 .. nv
__global__ void __launch_bounds__(kBlock)
corner_bounds_kernel(int nv, int64_t n3, const uint32_t* __restrict__ keys, uint32_t* __restrict__ start) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v > nv) return;
    uint32_t lo = 0u, hi = (uint32_t)n3;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < (uint32_t)v) lo = mid + 1u; else hi = mid;
    }
    start[v] = lo;
}

struct D3 { double x, y, z; };
__device__ __forceinline__ D3 load_d3(const float* __restrict__ p, int i) {
    D3 r;
    r.x = (double)p[3 * (int64_t)i]; r.y = (double)p[3 * (int64_t)i + 1]; r.z = (double)p[3 * (int64_t)i + 2];
    return r;
}

// N = sum over the vertex's faces, ascending, of (b - a) x (c - a) in the face's own corner order; n = N / sqrt(N.N), one rounding to fp32
__global__ void __launch_bounds__(kBlock)
vertex_normals_kernel(int nv, const float* __restrict__ vertices, const int32_t* __restrict__ faces, const uint32_t* __restrict__ corners,
                      const uint32_t* __restrict__ start, float* __restrict__ normals) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    double nx = 0.0, ny = 0.0, nz = 0.0;
    const uint32_t end = start[v + 1];
    for (uint32_t i = start[v]; i < end; ++i) {
        const int64_t f = corners[i] / 3u;
        const D3 a = load_d3(vertices, faces[3 * f]), b = load_d3(vertices, faces[3 * f + 1]), c = load_d3(vertices, faces[3 * f + 2]);
        const double ux = b.x - a.x, uy = b.y - a.y, uz = b.z - a.z, wx = c.x - a.x, wy = c.y - a.y, wz = c.z - a.z;
        nx = nx + (uy * wz - uz * wy);
        ny = ny + (uz * wx - ux * wz);
        nz = nz + (ux * wy - uy * wx);
    }
    float ox = 0.f, oy = 0.f, oz = 0.f;
    if (!(nx == 0.0 && ny == 0.0 && nz == 0.0)) {
        const double len = sqrt((nx * nx + ny * ny) + nz * nz);
        ox = (float)(nx / len); oy = (float)(ny / len); oz = (float)(nz / len);
    }
    normals[3 * v] = ox; normals[3 * v + 1] = oy; normals[3 * v + 2] = oz;
}

// one step: S = sum over the vertex's faces, ascending, of (p_j + p_k), the two corners after the vertex in the face's cyclic order; m = S / (2 |F|);
// p' = p + w (m - p), one rounding to fp32.  A vertex without a face keeps its bits.
__global__ void __launch_bounds__(kBlock)
smooth_step_kernel(int nv, const float* __restrict__ src, const int32_t* __restrict__ faces, const uint32_t* __restrict__ corners,
                   const uint32_t* __restrict__ start, float weight, float* __restrict__ dst) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v >= nv) return;
    const uint32_t first = start[v], end = start[v + 1];
    if (first == end) {
#pragma unroll
        for (int k = 0; k < 3; ++k) dst[3 * v + k] = src[3 * v + k];
        return;
    }
    double sx = 0.0, sy = 0.0, sz = 0.0;
    for (uint32_t i = first; i < end; ++i) {
        const uint32_t corner = corners[i];
        const int64_t f = corner / 3u;
        const int k = (int)(corner - 3u * (uint32_t)f);
        const D3 pj = load_d3(src, faces[3 * f + (k + 1) % 3]), pk = load_d3(src, faces[3 * f + (k + 2) % 3]);
        sx = sx + (pj.x + pk.x);
        sy = sy + (pj.y + pk.y);
        sz = sz + (pj.z + pk.z);
    }
    const double den = 2.0 * (double)(end - first), w = (double)weight;
    const D3 p = load_d3(src, (int)v);
    dst[3 * v] = (float)(p.x + w * (sx / den - p.x));
    dst[3 * v + 1] = (float)(p.y + w * (sy / den - p.y));
    dst[3 * v + 2] = (float)(p.z + w * (sz / den - p.z));
}

// corners sorted by vertex + the start table; returns the sorted corner list
const uint32_t* build_incidence(int nv, int nf, const int32_t* faces, MeshopsScratch& m, hipStream_t st) {
    const int64_t n3 = 3 * (int64_t)nf;
    hipLaunchKernelGGL(corner_keys_kernel, dim3(blocks_for(nf)), dim3(kBlock), 0, st, nv, (int64_t)nf, faces, m.keys[0], m.vals[0]);
    int nbits = 1;
    while (nbits < 32 && (1ull << nbits) <= (unsigned long long)nv) ++nbits;      // keys 0 .. nv
    const int cur = gsr_radix_sort_pairs(m.keys, m.vals, n3, nbits, 8, m.sort_hist, m.digit_total, sort_items(n3), st);
    hipLaunchKernelGGL(corner_bounds_kernel, dim3(blocks_for((int64_t)nv + 1)), dim3(kBlock), 0, st, nv, n3, (const uint32_t*)m.keys[cur], m.start);
    return m.vals[cur];
}

__global__ void __launch_bounds__(kBlock)
zero_start_kernel(int nv, uint32_t* __restrict__ start) {
    const int64_t v = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    if (v <= nv) start[v] = 0u;
}

}  // namespace

size_t gsr_meshops_scratch_bytes_impl(int nv, int nf) { return carve(nullptr, nv, nf).bytes + 128; }

int gsr_meshops_round_cap(int nv) {
    int lg = 0;
    while (((int64_t)1 << lg) < (int64_t)nv + 1) ++lg;
    return 2 * lg + 8;
}

int gsr_launch_mesh_components(int nv, int nf, const int32_t* faces, int32_t* vertex_label, int32_t* face_count, void* scratch, hipStream_t st,
                               int* rounds_out) {
    const MeshopsScratch m = carve(scratch, nv, nf);
    hipLaunchKernelGGL(cc_init_kernel, dim3(blocks_for(nv)), dim3(kBlock), 0, st, nv, vertex_label, face_count, m.word);
    const int cap = gsr_meshops_round_cap(nv);
    int round = 0;
    bool done = nf == 0;
    while (!done && round < cap) {
        ++round;
        hipLaunchKernelGGL(cc_hook_kernel, dim3(blocks_for(nf)), dim3(kBlock), 0, st, nv, (int64_t)nf, faces, vertex_label, m.word, (uint32_t)round);
        hipLaunchKernelGGL(cc_compress_kernel, dim3(blocks_for(nv)), dim3(kBlock), 0, st, nv, vertex_label);
        uint32_t last = 0;
        if (hipMemcpyAsync(&last, m.word, sizeof(last), hipMemcpyDeviceToHost, st) != hipSuccess || hipStreamSynchronize(st) != hipSuccess) return -1;
        done = last != (uint32_t)round;      // a round that hooked nothing: the fixpoint
    }
    if (rounds_out) *rounds_out = round;
    if (!done) return 1;
    if (nf > 0)
        hipLaunchKernelGGL(cc_face_count_kernel, dim3(blocks_for(nf)), dim3(kBlock), 0, st, nv, (int64_t)nf, faces, (const int32_t*)vertex_label,
                           face_count);
    return hipStreamSynchronize(st) == hipSuccess ? 0 : -1;
}

void gsr_launch_mesh_compact_count(int nv, int nf, const int32_t* faces, const uint8_t* keep, void* scratch, int32_t* counts_out, hipStream_t st) {
    const MeshopsScratch m = carve(scratch, nv, nf);
    if (nv > 0) hipLaunchKernelGGL(compact_clear_kernel, dim3(blocks_for(nv)), dim3(kBlock), 0, st, nv, m.mark);
    if (nf > 0 && nv > 0) hipLaunchKernelGGL(compact_mark_kernel, dim3(blocks_for(nf)), dim3(kBlock), 0, st, nv, (int64_t)nf, faces, keep, m.mark);
    hipLaunchKernelGGL(compact_count_kernel, dim3(m.nb), dim3(kBlock), 0, st, nv, (int64_t)nf, faces, keep, m);
    gsr_launch_rs_scan(m.hist, m.nb, 2, (uint32_t*)counts_out, st);      // in place: the workgroups' bases; the two row totals are the counts
}

void gsr_launch_mesh_compact_emit(int nv, int nf, const float* vertices, const float* colors, const int32_t* faces, const uint8_t* keep,
                                  void* scratch, int nv_out, int nf_out, float* vertices_out, float* colors_out, int32_t* faces_out, hipStream_t st) {
    const MeshopsScratch m = carve(scratch, nv, nf);
    if (colors && colors_out)
        hipLaunchKernelGGL(compact_emit_vertices_kernel<true>, dim3(blocks_for(nv)), dim3(kBlock), 0, st, nv, m, vertices, colors, nv_out, vertices_out,
                           colors_out);
    else
        hipLaunchKernelGGL(compact_emit_vertices_kernel<false>, dim3(blocks_for(nv)), dim3(kBlock), 0, st, nv, m, vertices, colors, nv_out, vertices_out,
                           colors_out);
    if (nf_out > 0 && nf > 0)
        hipLaunchKernelGGL(compact_emit_faces_kernel, dim3(blocks_for(nf)), dim3(kBlock), 0, st, nv, (int64_t)nf, m, faces, keep, nf_out, faces_out);
}

void gsr_launch_mesh_vertex_normals(int nv, int nf, const float* vertices, const int32_t* faces, float* normals, void* scratch, hipStream_t st) {
    MeshopsScratch m = carve(scratch, nv, nf);
    const uint32_t* corners = m.vals[0];
    if (nf > 0) corners = build_incidence(nv, nf, faces, m, st);
    else hipLaunchKernelGGL(zero_start_kernel, dim3(blocks_for((int64_t)nv + 1)), dim3(kBlock), 0, st, nv, m.start);
    hipLaunchKernelGGL(vertex_normals_kernel, dim3(blocks_for(nv)), dim3(kBlock), 0, st, nv, vertices, faces, corners, (const uint32_t*)m.start, normals);
}

void gsr_launch_mesh_smooth(int nv, int nf, const float* vertices, const int32_t* faces, int iterations, float lambda, float mu, float* vertices_out,
                            void* scratch, hipStream_t st) {
    MeshopsScratch m = carve(scratch, nv, nf);
    const uint32_t* corners = m.vals[0];
    if (nf > 0) corners = build_incidence(nv, nf, faces, m, st);
    else hipLaunchKernelGGL(zero_start_kernel, dim3(blocks_for((int64_t)nv + 1)), dim3(kBlock), 0, st, nv, m.start);
    // 2 * iterations steps, lambda then mu, ping-pong between the scratch buffer and the output so that the last step lands in the output
    const float* src = vertices;
    for (int s = 0; s < 2 * iterations; ++s) {
        float* dst = ((2 * iterations - 1 - s) & 1) ? m.tmp : vertices_out;
        hipLaunchKernelGGL(smooth_step_kernel, dim3(blocks_for(nv)), dim3(kBlock), 0, st, nv, src, faces, corners, (const uint32_t*)m.start,
                           (s & 1) ? mu : lambda, dst);
        src = dst;
    }
}
