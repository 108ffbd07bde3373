// TSDF fusion of rendered depth maps and mesh extraction by marching tetrahedra: the last step of the geometry line (2DGS, GOF,
// RaDe-GS, PGSR all end with it).  include/gsr.h states the semantics; this file the two native pieces.
//
// tsdf_integrate -- a voxel x camera sweep of the shape of mip.hip's: ONE kernel over all V views, so the volume is read and written at most once
// per call.  A wave owns a brick of 64 x 2 x 2 voxels, lanes along x (the depth gathers of a wave fall on neighbouring pixels), four voxels per
// lane; the camera records sit at wave-uniform addresses and arrive by scalar loads.  Per view the wave first bounds its brick in camera space
// (the box's centre through the record, its half extents through |R|: interval arithmetic, valid for any R) and skips the view when the record is
// not finite, the whole brick is behind `near`, or the whole brick projects off one side of the image -- the test is the same in every lane.
// Per (voxel, view) pair: three explicit fmaf chains, two correctly rounded divisions for the pixel, the gather, one more for sdf / trunc.  Every
// operation that decides something is a single correctly rounded fp32 operation, so the host build takes the same decisions as the device.  The
// running sums are added in view order; no atomics, two runs give the same bits.
// (A skip of bricks that lie wholly BEHIND a view's truncation band needs a bound on the view's depth, i.e. a pass over the depth stack and a
// buffer to keep it in; the entry point has no scratch and this file does not do it.)
//
// mesh_* -- marching tetrahedra on the dense volume as count -> scan -> emit, indexed without hashing: every edge of the six Kuhn tetrahedra of a
// cell runs from a grid point in one of seven directions, so a mesh vertex IS (owner voxel, direction).
//     mesh_classify   one byte per voxel: inside, observed, "the cell at this voxel is valid"
//     mesh_count      per voxel the 7-bit mask of owned vertices and the faces of its cell; their exclusive prefixes inside the workgroup (16 bits
//                     each) and the workgroup's totals, which sort.hip's rs_scan turns into bases and the two counts
//     mesh_emit       vertices by (owner, direction), faces by (cell, tetrahedron, face); a face finds a vertex's index from the owner's base,
//                     prefix and mask
// The 16 cases of a tetrahedron are derived, not tabulated: with the inside corners a (b) and the others in ascending order, the triangle
// (e_ab, e_ac, e_ad) -- the quad (e_ac, e_ad, e_bd, e_bc) for two inside corners -- faces outward in a positively oriented tetrahedron when the
// permutation (a, b, c, d) is even; an odd permutation, a negatively oriented tetrahedron and "three inside" (the lone corner is the OUTSIDE one)
// flip it once each.  Nothing looks at the computed geometry, so exact zeros and zero-area faces keep their winding.
#include "gsr_internal.h"
#include "gsr_wave.h"

namespace {

constexpr int kBlock = 256;
constexpr float kFltMax = 3.402823466e38f;
constexpr float kCullPad = 1e-5f;        // ~84 eps of the magnitudes that enter a camera-space coordinate: the rounding of both sides of a cull test

__device__ __forceinline__ bool finite1(float x) { return fabsf(x) <= kFltMax; }      // false for NaN and +-inf

struct TsdfGrid {
    int nx, ny, nz;
    float ox, oy, oz, voxel, trunc, near_z;
};

// ---- integrate ---------------------------------------------------------------------------------------------------------------------------
constexpr int kBrickX = 64, kBrickY = 2, kBrickZ = 2, kItems = kBrickY * kBrickZ;

template <bool COLOR>
__global__ void __launch_bounds__(kBlock)
tsdf_integrate_kernel(TsdfGrid g, int bx, int by, int64_t bricks, int V, const float* __restrict__ cams, int H, int W,
                      const float* __restrict__ depth, const float* __restrict__ color, float* __restrict__ tsdf, float* __restrict__ weight,
                      float* __restrict__ rgb) {
    const int wave = __builtin_amdgcn_readlane((int)(threadIdx.x >> 6), 0), lane = (int)(threadIdx.x & 63);
    int64_t brick = (int64_t)blockIdx.x * (kBlock / 64) + wave;
    if (brick >= bricks) brick = bricks - 1;      // (a wave past the end redoes the last brick's arithmetic and writes nothing)
    const bool live_wave = (int64_t)blockIdx.x * (kBlock / 64) + wave < bricks;
    const int x0 = (int)(brick % bx) * kBrickX, y0 = (int)((brick / bx) % by) * kBrickY, z0 = (int)(brick / ((int64_t)bx * by)) * kBrickZ;
    // the brick's box in world space (clipped to the volume): centre and half extents
    const int x1 = min(x0 + kBrickX, g.nx) - 1, y1 = min(y0 + kBrickY, g.ny) - 1, z1 = min(z0 + kBrickZ, g.nz) - 1;
    const float cwx = fmaf(g.voxel, 0.5f * (float)(x0 + x1), g.ox), cwy = fmaf(g.voxel, 0.5f * (float)(y0 + y1), g.oy);
    const float cwz = fmaf(g.voxel, 0.5f * (float)(z0 + z1), g.oz);
    const float hx = g.voxel * (0.5f * (float)(x1 - x0)), hy = g.voxel * (0.5f * (float)(y1 - y0)), hz = g.voxel * (0.5f * (float)(z1 - z0));

    const int ix = x0 + lane;
    float px[kItems], py[kItems], pz[kItems], s[kItems], c0[kItems], c1[kItems], c2[kItems];
    int n[kItems];
    bool live[kItems];
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        const int iy = y0 + (k & 1), iz = z0 + (k >> 1);
        live[k] = live_wave && ix < g.nx && iy < g.ny && iz < g.nz;
        px[k] = fmaf(g.voxel, (float)ix, g.ox); py[k] = fmaf(g.voxel, (float)iy, g.oy); pz[k] = fmaf(g.voxel, (float)iz, g.oz);
        s[k] = 0.f; n[k] = 0; c0[k] = c1[k] = c2[k] = 0.f;
    }
    const float half_w = 0.5f * (float)W, half_h = 0.5f * (float)H, wf = (float)W, hf = (float)H;
    const int64_t plane = (int64_t)H * W;

    for (int v = 0; v < V; ++v) {
        // wave-uniform: one 64-byte scalar load.  (Loading the record of view v + 1 while view v is worked on was measured and is not faster,
        // eight waves per SIMD hide the load already.)
        const float* __restrict__ r = cams + 16 * (int64_t)v;
        const float r00 = r[0], r01 = r[1], r02 = r[2], r10 = r[3], r11 = r[4], r12 = r[5], r20 = r[6], r21 = r[7], r22 = r[8];
        const float t0 = r[9], t1 = r[10], t2 = r[11], fx = r[12], fy = r[13];
        // ---- the brick against this view: the same values in every lane ----
        float fin = 0.f;      // x * 0 is 0 for a finite x and NaN otherwise
#pragma unroll
        for (int i = 0; i < 16; ++i) fin = fmaf(r[i], 0.f, fin);
        const float bz = fmaf(cwx, r02, fmaf(cwy, r12, fmaf(cwz, r22, t2)));
        const float bxc = fmaf(cwx, r00, fmaf(cwy, r10, fmaf(cwz, r20, t0)));
        const float byc = fmaf(cwx, r01, fmaf(cwy, r11, fmaf(cwz, r21, t1)));
        const float ez = fmaf(hx, fabsf(r02), fmaf(hy, fabsf(r12), hz * fabsf(r22)));      // half extents of the box's image in camera space
        const float ex = fmaf(hx, fabsf(r00), fmaf(hy, fabsf(r10), hz * fabsf(r20)));
        const float ey = fmaf(hx, fabsf(r01), fmaf(hy, fabsf(r11), hz * fabsf(r21)));
        const float mz = fmaf(fabsf(cwx), fabsf(r02), fmaf(fabsf(cwy), fabsf(r12), fmaf(fabsf(cwz), fabsf(r22), fabsf(t2)))) + ez;
        const float mx = fmaf(fabsf(cwx), fabsf(r00), fmaf(fabsf(cwy), fabsf(r10), fmaf(fabsf(cwz), fabsf(r20), fabsf(t0)))) + ex;
        const float my = fmaf(fabsf(cwx), fabsf(r01), fmaf(fabsf(cwy), fabsf(r11), fmaf(fabsf(cwz), fabsf(r21), fabsf(t1)))) + ey;
        const float zhi = bz + ez + kCullPad * mz;                       // no voxel of the brick has a larger z
        const float xlo = fabsf(bxc) - ex - kCullPad * mx;               // ... or a smaller |x|, |y|
        const float ylo = fabsf(byc) - ey - kCullPad * my;
        // a pixel inside the image needs |fx x| <= W / 2 z and |fy y| <= H / 2 z; (1 + 2 pad) covers the roundings of the products
        const bool see = (fin == 0.f) & (zhi > g.near_z) & !(fabsf(fx) * xlo > half_w * zhi * (1.f + 2.f * kCullPad)) &
                         !(fabsf(fy) * ylo > half_h * zhi * (1.f + 2.f * kCullPad));
        if (!see) continue;
        float zk[kItems];
        int64_t at[kItems];
        bool on[kItems];
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            const float z = fmaf(px[k], r02, fmaf(py[k], r12, fmaf(pz[k], r22, t2)));      // cam = xyz R + T
            const float x = fmaf(px[k], r00, fmaf(py[k], r10, fmaf(pz[k], r20, t0)));
            const float y = fmaf(px[k], r01, fmaf(py[k], r11, fmaf(pz[k], r21, t1)));
            const float u = __fadd_rn(__fdiv_rn(__fmul_rn(fx, x), z), half_w);
            const float w = __fadd_rn(__fdiv_rn(__fmul_rn(fy, y), z), half_h);
            // floor(u) in [0, W) <=> 0 <= u < W; a NaN fails every comparison
            on[k] = live[k] & (z > g.near_z) & (z <= kFltMax) & (u >= 0.f) & (u < wf) & (w >= 0.f) & (w < hf);
            // (the conversions truncate, which is floor for u, w >= 0; below W, H by the test; a pair that is not `on` reads pixel 0 and drops it)
            at[k] = (int64_t)v * plane + (on[k] ? (int64_t)(int)w * W + (int)u : 0);
            zk[k] = z;
        }
        float d[kItems];
#pragma unroll
        for (int k = 0; k < kItems; ++k) d[k] = depth[at[k]];      // unconditional: the four gathers are in flight together
#pragma unroll
        for (int k = 0; k < kItems; ++k) {
            const float sdf = __fsub_rn(d[k], zk[k]);
            const bool take = on[k] & (d[k] > 0.f) & (d[k] <= kFltMax) & (sdf >= -g.trunc);
            if (take) {
                s[k] = __fadd_rn(s[k], fminf(1.f, __fdiv_rn(sdf, g.trunc)));
                n[k] += 1;
                if (COLOR) {
                    const float* cv = color + 2 * (int64_t)v * plane + at[k];      // (at holds v * plane already)
                    c0[k] = __fadd_rn(c0[k], cv[0]); c1[k] = __fadd_rn(c1[k], cv[plane]); c2[k] = __fadd_rn(c2[k], cv[2 * plane]);
                }
            }
        }
    }
    // the volume: read (at a clamped address, all together) and, where a view observed the voxel, written -- once per call
    const int64_t cells = (int64_t)g.nx * g.ny * g.nz;
    int64_t vi[kItems];
    float t_old[kItems], w_old[kItems], r_old[kItems], g_old[kItems], b_old[kItems];
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        const bool hit = live[k] && n[k] > 0;
        vi[k] = hit ? ((int64_t)(z0 + (k >> 1)) * g.ny + (y0 + (k & 1))) * g.nx + ix : 0;
        t_old[k] = tsdf[vi[k]]; w_old[k] = weight[vi[k]];
        if (COLOR) { r_old[k] = rgb[vi[k]]; g_old[k] = rgb[cells + vi[k]]; b_old[k] = rgb[2 * cells + vi[k]]; }
    }
#pragma unroll
    for (int k = 0; k < kItems; ++k) {
        if (!live[k] || n[k] == 0) continue;      // a voxel no view of the call observed is not written
        const float w_new = __fadd_rn(w_old[k], (float)n[k]);
        tsdf[vi[k]] = __fdiv_rn(__fadd_rn(__fmul_rn(t_old[k], w_old[k]), s[k]), w_new);
        if (COLOR) {
            rgb[vi[k]] = __fdiv_rn(__fadd_rn(__fmul_rn(r_old[k], w_old[k]), c0[k]), w_new);
            rgb[cells + vi[k]] = __fdiv_rn(__fadd_rn(__fmul_rn(g_old[k], w_old[k]), c1[k]), w_new);
            rgb[2 * cells + vi[k]] = __fdiv_rn(__fadd_rn(__fmul_rn(b_old[k], w_old[k]), c2[k]), w_new);
        }
        weight[vi[k]] = w_new;
    }
}

// ---- marching tetrahedra -------------------------------------------------------------------------------------------------------------------
// A corner of a cell, and an edge direction, is a 3-bit code (x = 1, y = 2, z = 4).  Directions 0..6 are (1,0,0), (0,1,0), (0,0,1), (1,1,0), (1,0,1),
// (0,1,1), (1,1,1): codes 1, 2, 4, 3, 5, 6, 7.  The Kuhn tetrahedron of the axis permutation pi has the corners 0, e_pi1, e_pi1 + e_pi2, 7 and the
// orientation of pi; the six permutations in lexicographic order:
constexpr uint32_t kDirCode = 0x7653421u;          // nibble d: the code of direction d
constexpr uint32_t kCodeDir = 0x65423100u;         // nibble c: the direction of code c
constexpr uint32_t kTetV1 = 0x442211u;             // nibble t: corner 1 of tetrahedron t (xyz, xzy, yxz, yzx, zxy, zyx)
constexpr uint32_t kTetV2 = 0x656353u;             // nibble t: corner 2
constexpr uint32_t kTetOdd = 0x26u;                // bit t: pi is odd, the tetrahedron is negatively oriented
constexpr uint64_t kEdgeCells = 0x0103050F11335500ull;      // byte c: the cells p - o (bit o) that contain the edge from p with direction code c: o & c == 0

constexpr uint8_t kInside = 1, kObserved = 2, kCellValid = 4;

struct MeshScratch {
    uint32_t* hist;       // [2][nb]: vertices, faces per workgroup -> exclusive bases (rs_scan)
    uint16_t* vloc;       // [nb * 256] exclusive prefix of the voxel's vertices inside its workgroup
    uint16_t* floc;       // [nb * 256] ... of its cell's faces
    uint8_t* cls;         // [nb * 256]
    uint8_t* mask;        // [nb * 256] bit d: the voxel owns a vertex in direction d
    int nb;
};

__device__ __forceinline__ int nib(uint32_t table, int i) { return (int)((table >> (4 * i)) & 15u); }

// the faces of one tetrahedron: m = its inside corners (bit k: corner k).  Returns the number of faces (0..2).  An edge is (low corner << 2 | high
// corner), corners numbered 0..3 inside the tetrahedron; a face is its three edges in three nibbles (vertex j: bits 4 j .. 4 j + 3), so that nothing
// here is an array the compiler would have to index at run time (it put one into LDS).
__device__ __forceinline__ int tet_faces(int m, bool odd_tet, int& face0, int& face1) {
    const int cnt = __popc(m);
    face0 = face1 = 0;
    if (cnt == 0 || cnt == 4) return 0;
    auto edge = [](int p, int q) { return p < q ? (p << 2 | q) : (q << 2 | p); };
    if (cnt != 2) {
        const int lone = cnt == 1 ? m : (~m & 15);
        const int a = 31 - __clz(lone);                          // the lone corner; (a, others ascending) is a permutation of parity a
        const int b = a == 0 ? 1 : 0, c = a <= 1 ? 2 : 1, d = a == 3 ? 2 : 3;
        const bool flip = ((a & 1) != 0) ^ odd_tet ^ (cnt == 3);
        face0 = edge(a, b) | (flip ? edge(a, d) : edge(a, c)) << 4 | (flip ? edge(a, c) : edge(a, d)) << 8;
        return 1;
    }
    const int a = __ffsll((unsigned long long)m) - 1, b = 31 - __clz(m);      // inside a < b
    const int o = ~m & 15;
    const int c = __ffsll((unsigned long long)o) - 1, d = 31 - __clz(o);      // outside c < d; (a, b, c, d) has a + b - 1 inversions
    const bool flip = (((a + b - 1) & 1) != 0) ^ odd_tet;
    const int q0 = edge(a, c), q1 = flip ? edge(b, c) : edge(a, d), q2 = edge(b, d), q3 = flip ? edge(a, d) : edge(b, c);
    face0 = q0 | q1 << 4 | q2 << 8;
    face1 = q0 | q2 << 4 | q3 << 8;
    return 2;
}

__device__ __forceinline__ int tet_corner(int t, int k) { return k == 0 ? 0 : k == 1 ? nib(kTetV1, t) : k == 2 ? nib(kTetV2, t) : 7; }

__device__ __forceinline__ int tet_mask(int ins, int t) {      // ins: bit c = corner code c of the cell is inside
    return (ins & 1) | ((ins >> nib(kTetV1, t)) & 1) << 1 | ((ins >> nib(kTetV2, t)) & 1) << 2 | ((ins >> 7) & 1) << 3;
}

struct Voxel { int64_t i; int x, y, z; bool in; };

__device__ __forceinline__ Voxel voxel_of_thread(const TsdfGrid& g, int64_t cells) {
    Voxel p;
    p.i = (int64_t)blockIdx.x * kBlock + threadIdx.x;
    p.in = p.i < cells;
    const int64_t j = p.in ? p.i : 0;
    p.x = (int)(j % g.nx); p.y = (int)((j / g.nx) % g.ny); p.z = (int)(j / ((int64_t)g.nx * g.ny));
    return p;
}

__device__ __forceinline__ int64_t step(const TsdfGrid& g, int code) {      // the index offset of a corner / direction code
    return (code & 1) + (int64_t)((code >> 1) & 1) * g.nx + (int64_t)((code >> 2) & 1) * g.nx * g.ny;
}

__global__ void __launch_bounds__(kBlock)
mesh_classify_kernel(TsdfGrid g, int64_t cells, const float* __restrict__ tsdf, const float* __restrict__ weight, float min_weight,
                     uint8_t* __restrict__ cls) {
    const Voxel p = voxel_of_thread(g, cells);
    if (!p.in) { cls[p.i] = 0; return; }      // (the tables are padded to whole workgroups)
    const bool cell = p.x + 1 < g.nx && p.y + 1 < g.ny && p.z + 1 < g.nz;
    bool all = cell;
    uint8_t own = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) {
        if (c > 0 && !cell) break;
        const int64_t q = p.i + step(g, c);
        const float s = tsdf[q];
        const bool obs = (weight[q] >= min_weight) & finite1(s);
        if (c == 0) own = (uint8_t)((s < 0.f ? kInside : 0) | (obs ? kObserved : 0));
        all = all & obs;
    }
    cls[p.i] = (uint8_t)(own | (all ? kCellValid : 0));
}

// bit c of the result: corner code c of the cell at p is inside (p's cell must exist)
__device__ __forceinline__ int cell_inside_bits(const TsdfGrid& g, const Voxel& p, const uint8_t* __restrict__ cls) {
    int ins = 0;
#pragma unroll
    for (int c = 0; c < 8; ++c) ins |= (int)(cls[p.i + step(g, c)] & kInside) << c;
    return ins;
}

__global__ void __launch_bounds__(kBlock)
mesh_count_kernel(TsdfGrid g, int64_t cells, MeshScratch m) {
    __shared__ uint32_t wsum[gsrw::WG_WAVES];
    const Voxel p = voxel_of_thread(g, cells);
    int vmask = 0, faces = 0;
    if (p.in) {
        // fifteen bytes around the voxel, every one from an address inside the table (the voxel's own where the neighbour does not exist): the
        // loads are unconditional and in flight together
        uint8_t below[8], above[8];
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            const bool lo = p.x >= (o & 1) && p.y >= ((o >> 1) & 1) && p.z >= ((o >> 2) & 1);
            const bool hi = p.x + (o & 1) < g.nx && p.y + ((o >> 1) & 1) < g.ny && p.z + ((o >> 2) & 1) < g.nz;
            below[o] = m.cls[lo ? p.i - step(g, o) : p.i];
            above[o] = m.cls[hi ? p.i + step(g, o) : p.i];
            if (!lo) below[o] = 0;      // (no such cell)
        }
        const uint8_t own = above[0];
        int valid_cells = 0, ins = 0;      // bit o: the cell at p - o is valid;  bit c: the voxel at p + c is inside
#pragma unroll
        for (int o = 0; o < 8; ++o) {
            valid_cells |= (int)((below[o] >> 2) & 1) << o;
            ins |= (int)(above[o] & kInside) << o;
        }
#pragma unroll
        for (int d = 0; d < 7; ++d) {
            const int c = nib(kDirCode, d);
            // (a valid cell holds both ends of the edge: where one contains it, the far end exists and above[c] is its byte)
            if (valid_cells & (int)((kEdgeCells >> (8 * c)) & 0xFFu)) vmask |= (((ins >> c) ^ ins) & 1) << d;
        }
        if (own & kCellValid) {
#pragma unroll
            for (int t = 0; t < 6; ++t) {
                const int cnt = __popc(tet_mask(ins, t));
                faces += cnt == 2 ? 2 : (cnt == 1 || cnt == 3) ? 1 : 0;
            }
        }
    }
    // both counts through one scan: at most 7 * 256 vertices and 12 * 256 faces per workgroup, 16 bits each
    const uint32_t v[1] = {(uint32_t)__popc(vmask) | (uint32_t)faces << 16};
    const uint32_t excl = gsrw::block_excl_scan<1>(v, wsum, (int)(threadIdx.x & 63), (int)(threadIdx.x >> 6));
    m.mask[p.i] = (uint8_t)vmask;
    m.vloc[p.i] = (uint16_t)(excl & 0xFFFFu);
    m.floc[p.i] = (uint16_t)(excl >> 16);
    if (threadIdx.x == kBlock - 1) {
        const uint32_t total = excl + v[0];
        m.hist[blockIdx.x] = total & 0xFFFFu;
        m.hist[m.nb + blockIdx.x] = total >> 16;
    }
}

template <bool COLOR>
__global__ void __launch_bounds__(kBlock)
mesh_emit_kernel(TsdfGrid g, int64_t cells, MeshScratch m, const float* __restrict__ tsdf, const float* __restrict__ rgb, int nv, int nf,
                 float* __restrict__ vertices, float* __restrict__ colors, int32_t* __restrict__ faces) {
    const Voxel p = voxel_of_thread(g, cells);
    if (!p.in) return;
    const int vmask = m.mask[p.i];
    if (vmask) {
        int64_t at = (int64_t)m.hist[blockIdx.x] + m.vloc[p.i];
        const float s0 = tsdf[p.i];
        const float x = fmaf(g.voxel, (float)p.x, g.ox), y = fmaf(g.voxel, (float)p.y, g.oy), z = fmaf(g.voxel, (float)p.z, g.oz);
        float s1[7];
#pragma unroll
        for (int d = 0; d < 7; ++d) s1[d] = tsdf[((vmask >> d) & 1) ? p.i + step(g, nib(kDirCode, d)) : p.i];      // together, from addresses that exist
#pragma unroll
        for (int d = 0; d < 7; ++d) {
            if (!((vmask >> d) & 1)) continue;
            const int c = nib(kDirCode, d);
            const int64_t q = p.i + step(g, c);
            const float t = __fdiv_rn(s0, __fsub_rn(s0, s1[d]));      // the ends differ in sign class: the difference is not zero
            if (at < nv) {                                               // (a caller's nv below the count must not write past its buffer)
                vertices[3 * at] = __fadd_rn(x, __fmul_rn(t, (c & 1) ? g.voxel : 0.f));
                vertices[3 * at + 1] = __fadd_rn(y, __fmul_rn(t, (c & 2) ? g.voxel : 0.f));
                vertices[3 * at + 2] = __fadd_rn(z, __fmul_rn(t, (c & 4) ? g.voxel : 0.f));
                if (COLOR) {
#pragma unroll
                    for (int ch = 0; ch < 3; ++ch) {
                        const float a = rgb[ch * cells + p.i], b = rgb[ch * cells + q];
                        colors[3 * at + ch] = __fadd_rn(a, __fmul_rn(t, __fsub_rn(b, a)));
                    }
                }
            }
            ++at;
        }
    }
    if (!(m.cls[p.i] & kCellValid)) return;
    const int ins = cell_inside_bits(g, p, m.cls);
    if (ins == 0 || ins == 255) return;
    int64_t at = (int64_t)m.hist[m.nb + blockIdx.x] + m.floc[p.i];
    for (int t = 0; t < 6; ++t) {
        int face0, face1;
        const int count = tet_faces(tet_mask(ins, t), (kTetOdd >> t) & 1, face0, face1);
        for (int f = 0; f < count; ++f) {
            const int face = f ? face1 : face0;
            int32_t id[3];
#pragma unroll
            for (int j = 0; j < 3; ++j) {
                const int e = (face >> (4 * j)) & 15;
                const int lo = tet_corner(t, e >> 2), hi = tet_corner(t, e & 3);
                const int64_t owner = p.i + step(g, lo);
                const int d = nib(kCodeDir, hi - lo);      // (corner codes of a Kuhn tetrahedron ascend bitwise: hi - lo is the direction code)
                id[j] = (int32_t)(m.hist[owner / kBlock] + m.vloc[owner] + (uint32_t)__popc(m.mask[owner] & ((1 << d) - 1)));
            }
            if (at < nf) { faces[3 * at] = id[0]; faces[3 * at + 1] = id[1]; faces[3 * at + 2] = id[2]; }
            ++at;
        }
    }
}

inline int mesh_blocks(int nx, int ny, int nz) { return (int)(((int64_t)nx * ny * nz + kBlock - 1) / kBlock); }

inline MeshScratch carve(void* scratch, int nb) {
    MeshScratch m;
    char* p = (char*)scratch;
    const size_t padded = (size_t)nb * kBlock;
    m.nb = nb;
    m.hist = (uint32_t*)p; p += gsr_align128((size_t)2 * nb * sizeof(uint32_t));
    m.vloc = (uint16_t*)p; p += gsr_align128(padded * sizeof(uint16_t));
    m.floc = (uint16_t*)p; p += gsr_align128(padded * sizeof(uint16_t));
    m.cls = (uint8_t*)p; p += gsr_align128(padded);
    m.mask = (uint8_t*)p;
    return m;
}

inline TsdfGrid grid_of(int nx, int ny, int nz, float ox, float oy, float oz, float voxel, float trunc, float near_z) {
    TsdfGrid g;
    g.nx = nx; g.ny = ny; g.nz = nz; g.ox = ox; g.oy = oy; g.oz = oz; g.voxel = voxel; g.trunc = trunc; g.near_z = near_z;
    return g;
}

}  // namespace

void gsr_launch_tsdf_integrate(int nx, int ny, int nz, float ox, float oy, float oz, float voxel_size, float sdf_trunc, float near_z, int V,
                               const float* cameras, int H, int W, const float* depth, const float* color, float* tsdf, float* weight, float* rgb,
                               hipStream_t st) {
    const TsdfGrid g = grid_of(nx, ny, nz, ox, oy, oz, voxel_size, sdf_trunc, near_z);
    const int bx = (nx + kBrickX - 1) / kBrickX, by = (ny + kBrickY - 1) / kBrickY, bz = (nz + kBrickZ - 1) / kBrickZ;
    const int64_t bricks = (int64_t)bx * by * bz;
    const dim3 grid((unsigned)((bricks + kBlock / 64 - 1) / (kBlock / 64)));
    if (color && rgb)
        hipLaunchKernelGGL(tsdf_integrate_kernel<true>, grid, dim3(kBlock), 0, st, g, bx, by, bricks, V, cameras, H, W, depth, color, tsdf, weight, rgb);
    else
        hipLaunchKernelGGL(tsdf_integrate_kernel<false>, grid, dim3(kBlock), 0, st, g, bx, by, bricks, V, cameras, H, W, depth, color, tsdf, weight,
                           rgb);
}

size_t gsr_mesh_scratch_bytes_impl(int nx, int ny, int nz) {
    const int nb = mesh_blocks(nx, ny, nz);
    const size_t padded = (size_t)nb * kBlock;
    return gsr_align128((size_t)2 * nb * sizeof(uint32_t)) + 2 * gsr_align128(padded * sizeof(uint16_t)) + 2 * gsr_align128(padded) + 128;
}

void gsr_launch_mesh_count(int nx, int ny, int nz, const float* tsdf, const float* weight, float min_weight, void* scratch, int32_t* counts_out,
                           hipStream_t st) {
    const TsdfGrid g = grid_of(nx, ny, nz, 0.f, 0.f, 0.f, 1.f, 1.f, 0.f);
    const int nb = mesh_blocks(nx, ny, nz);
    const int64_t cells = (int64_t)nx * ny * nz;
    const MeshScratch m = carve(scratch, nb);
    hipLaunchKernelGGL(mesh_classify_kernel, dim3(nb), dim3(kBlock), 0, st, g, cells, tsdf, weight, min_weight, m.cls);
    hipLaunchKernelGGL(mesh_count_kernel, dim3(nb), dim3(kBlock), 0, st, g, cells, m);
    gsr_launch_rs_scan(m.hist, nb, 2, (uint32_t*)counts_out, st);      // in place: the workgroups' bases; the two row totals are the counts
}

void gsr_launch_mesh_emit(int nx, int ny, int nz, float ox, float oy, float oz, float voxel_size, const float* tsdf, const float* rgb,
                          void* scratch, int nv, int nf, float* vertices, float* colors, int32_t* faces, hipStream_t st) {
    const TsdfGrid g = grid_of(nx, ny, nz, ox, oy, oz, voxel_size, 1.f, 0.f);
    const int nb = mesh_blocks(nx, ny, nz);
    const int64_t cells = (int64_t)nx * ny * nz;
    const MeshScratch m = carve(scratch, nb);
    if (rgb && colors)
        hipLaunchKernelGGL(mesh_emit_kernel<true>, dim3(nb), dim3(kBlock), 0, st, g, cells, m, tsdf, rgb, nv, nf, vertices, colors, faces);
    else
        hipLaunchKernelGGL(mesh_emit_kernel<false>, dim3(nb), dim3(kBlock), 0, st, g, cells, m, tsdf, rgb, nv, nf, vertices, colors, faces);
}
