// lz_mesh.hip -- marching cubes on the lattice of extract_fields (nerf_triplane/utils.py:366-378: extract_geometry's
// mcubes.marching_cubes(u, threshold)) for gfx950.  The mesh is a function of (u, thr) alone, defined in DESIGN 4.13:
//
//   solid(v) = v >= thr.  Lattice edge (n, a), from node n = (i Ry + j) Rz + k to its +1 neighbour on axis a, is cut when its ends differ
//   in solid; its vertex sits at t = (thr - u_lo) / (u_hi - u_lo) from node n, clamped to [0, 1] (NaN -> 0), one f32 operation per
//   operator.  Vertex ids are the ranks of the keys 3 n + a of the cut edges.  Triangles are ordered by cell, inside a cell in the order
//   of the generated table (include/lzzx_mc_tables.h, tools/gen_mc_tables.py), and wind so that the normal points from solid to empty.
//
// Two passes over the lattice with a scan between them, every output position fixed by the scans (no atomics):
//
//   lz_k_mc_count  one workgroup per tile of LZM_TILE nodes of one lattice row (i, j, .).  Per node the 3-bit mask of owned cut edges
//                  and the cell's triangle count; a workgroup scan gives the node's vertex offset inside the tile.  Writes one 16-bit
//                  word per node, (tile-local vertex offset << 3) | cut mask, and the tile's (vertices, triangles) totals.
//   lz_k_mc_scan_tiles / lz_k_mc_scan   exclusive scan of the tile totals in place, in two levels: every LZM_SCAN_WG tiles by one
//                  workgroup (coalesced), then the groups' sums by one workgroup, which also hands the grand totals to the caller.
//                  A tile's base is its scanned total plus its group's.
//   lz_k_mc_emit   the same tiling and the same workgroup scan again (recomputed from u, not stored), plus the tile's base: each node
//                  writes its vertices, each cell its triangles.  A triangle's vertex on cell edge (node m, axis a) is
//                  base[tile(m)] + (word[m] >> 3) + popcount(word[m] & ((1 << a) - 1)): the scanned offsets plus the node's lower-axis
//                  cut edges, no hash.
//
// A thread loads the (up to) four nodes (i + dx, j + dy, k) of its column; the four at k + 1 come from its neighbour through LDS, so u is
// read four times per node from L1 / L2 and about once from HBM.  The table sits in LDS.
#define LZ_MC_TABLE_QUAL __constant__ const __attribute__((aligned(16)))
#include "lzzx_mc_tables.h"

#include "lz_common.h"

#define LZM_TILE 256          // nodes of a row per workgroup = threads per workgroup
#define LZM_SCAN_WG 1024      // threads of the one scan workgroup

struct LzmGeom {
    uint32_t Rx, Ry, Rz;
    uint32_t tiles;           // tiles per row, ceil(Rz / LZM_TILE)
};

// exclusive scan of v over the NW waves of the workgroup (wsum: NW words of LDS, used once per kernel); total = the workgroup's sum
template <int NW>
__device__ __forceinline__ uint32_t lzm_block_scan(uint32_t v, uint32_t* wsum, uint32_t& total) {
    const uint32_t lane = threadIdx.x & 63u, w = threadIdx.x >> 6;
    uint32_t incl = v;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t t = __shfl_up(incl, d, 64);
        if (lane >= (uint32_t)d) incl += t;
    }
    if (lane == 63) wsum[w] = incl;
    __syncthreads();
    uint32_t base = 0, all = 0;
#pragma unroll
    for (int x = 0; x < NW; x++) {
        const uint32_t s = wsum[x];
        if ((uint32_t)x < w) base += s;
        all += s;
    }
    total = all;
    return base + incl - v;
}

// what a thread knows about its node after the shared front half of both passes
struct LzmNode {
    uint32_t n, row, k;       // linear node index, row = i Ry + j, position in the row
    uint32_t sx, sy;          // node strides of axes 0 and 1
    uint32_t kase, cut, ntri; // the cell's case, the owned cut edges (bit a), the cell's triangles; all 0 for a thread outside the row
    float v00, v01, v10;      // u at the node and at its +1 neighbours on axes 1 and 0 (valid where that edge exists)
    uint32_t local_v, local_t, tile_v, tile_t;   // tile-local exclusive offsets and the tile's totals
};

__device__ __forceinline__ uint32_t lzm_column(const float* __restrict__ u, uint32_t n, uint32_t sx, uint32_t sy, bool hx, bool hy, float thr,
                                               float& v00, float& v01, float& v10) {
    uint32_t m = 0;
    v00 = u[n];
    m |= (uint32_t)(v00 >= thr);
    if (hy) { v01 = u[n + sy]; m |= (uint32_t)(v01 >= thr) << 1; }
    if (hx) {
        v10 = u[n + sx];
        m |= (uint32_t)(v10 >= thr) << 2;
        if (hy) m |= (uint32_t)(u[n + sx + sy] >= thr) << 3;
    }
    return m;
}

// bit p of x -> bit 2 p
__device__ __forceinline__ uint32_t lzm_spread(uint32_t x) { return (x & 1u) | (x & 2u) << 1 | (x & 4u) << 2 | (x & 8u) << 3; }

// nt[kase * stride + off] = triangles of a case.  sb: LZM_TILE + 1 bytes, wsum: LZM_TILE / 64 words of LDS
__device__ __forceinline__ void lzm_node(const float* __restrict__ u, const LzmGeom& g, float thr, const uint8_t* nt, uint32_t stride, uint32_t off,
                                         uint8_t* sb, uint32_t* wsum, LzmNode& nd) {
    const uint32_t tid = threadIdx.x;
    const uint32_t row = blockIdx.x / g.tiles, tz = blockIdx.x - row * g.tiles;
    const uint32_t i = row / g.Ry, j = row - i * g.Ry;
    const uint32_t k = tz * LZM_TILE + tid;
    const bool active = k < g.Rz, hx = i + 1 < g.Rx, hy = j + 1 < g.Ry, hz = k + 1 < g.Rz;
    nd.row = row; nd.k = k; nd.sy = g.Rz; nd.sx = g.Ry * g.Rz;
    nd.n = row * g.Rz + k;
    nd.v00 = nd.v01 = nd.v10 = 0.0f;
    uint32_t lo = 0;
    if (active) lo = lzm_column(u, nd.n, nd.sx, nd.sy, hx, hy, thr, nd.v00, nd.v01, nd.v10);
    sb[tid] = (uint8_t)lo;
    if (tid == LZM_TILE - 1) {       // the column behind the tile's last node
        uint32_t m = 0;
        float a, b, c;
        if (hz) m = lzm_column(u, nd.n + 1, nd.sx, nd.sy, hx, hy, thr, a, b, c);
        sb[LZM_TILE] = (uint8_t)m;
    }
    __syncthreads();
    const uint32_t hi = sb[tid + 1];
    nd.kase = lzm_spread(lo) | lzm_spread(hi) << 1;      // corner 4 dx + 2 dy + dz
    uint32_t cut = 0;
    if (active) {
        const uint32_t s = lo & 1u;
        if (hx && s != (lo >> 2 & 1u)) cut |= 1u;
        if (hy && s != (lo >> 1 & 1u)) cut |= 2u;
        if (hz && s != (hi & 1u)) cut |= 4u;
    }
    nd.cut = cut;
    nd.ntri = (active && hx && hy && hz) ? nt[nd.kase * stride + off] : 0u;
    // one scan for both counts: at most 3 * 256 vertices and 5 * 256 triangles per tile
    uint32_t total;
    const uint32_t ex = lzm_block_scan<LZM_TILE / 64>((uint32_t)__popc(cut) | nd.ntri << 16, wsum, total);
    nd.local_v = ex & 0xFFFFu; nd.local_t = ex >> 16;
    nd.tile_v = total & 0xFFFFu; nd.tile_t = total >> 16;
}

__global__ void __launch_bounds__(LZM_TILE)
lz_k_mc_count(const float* __restrict__ u, LzmGeom g, float thr, uint16_t* __restrict__ info, uint2* __restrict__ blk) {
    __shared__ uint8_t nt[256];
    __shared__ uint8_t sb[LZM_TILE + 1];
    __shared__ uint32_t wsum[LZM_TILE / 64];
    nt[threadIdx.x] = lz_mc_ntri[threadIdx.x];     // (LZM_TILE == 256; read behind the barrier inside lzm_node)
    LzmNode nd;
    lzm_node(u, g, thr, nt, 1, 0, sb, wsum, nd);
    if (nd.k < g.Rz) info[nd.n] = (uint16_t)(nd.local_v << 3 | nd.cut);
    if (threadIdx.x == 0) blk[blockIdx.x] = make_uint2(nd.tile_v, nd.tile_t);
}

// blk[b] = (vertices, triangles) of tile b -> the exclusive sums over the tiles before b IN ITS GROUP of LZM_SCAN_WG tiles, in place;
// aux[g] = the sums over group g
__global__ void __launch_bounds__(LZM_SCAN_WG)
lz_k_mc_scan_tiles(uint2* __restrict__ blk, uint32_t nb, uint2* __restrict__ aux) {
    __shared__ uint32_t wsum_v[LZM_SCAN_WG / 64], wsum_t[LZM_SCAN_WG / 64];
    const uint32_t b = blockIdx.x * LZM_SCAN_WG + threadIdx.x;
    const uint2 x = b < nb ? blk[b] : make_uint2(0u, 0u);
    uint32_t all_v, all_t;
    const uint32_t ev = lzm_block_scan<LZM_SCAN_WG / 64>(x.x, wsum_v, all_v);
    const uint32_t et = lzm_block_scan<LZM_SCAN_WG / 64>(x.y, wsum_t, all_t);
    if (b < nb) blk[b] = make_uint2(ev, et);
    if (threadIdx.x == 0) aux[blockIdx.x] = make_uint2(all_v, all_t);
}

// the same over the nb group sums, by ONE workgroup (consecutive spans per thread: any nb), in place; totals = the sums over everything
__global__ void __launch_bounds__(LZM_SCAN_WG)
lz_k_mc_scan(uint2* __restrict__ blk, uint32_t nb, uint32_t* __restrict__ totals) {
    __shared__ uint32_t wsum_v[LZM_SCAN_WG / 64], wsum_t[LZM_SCAN_WG / 64];
    const uint32_t span = (nb + LZM_SCAN_WG - 1) / LZM_SCAN_WG;      // consecutive tiles per thread
    const uint32_t lo = min(threadIdx.x * span, nb), hi = min(lo + span, nb);
    uint32_t sv = 0, st = 0;
    for (uint32_t b = lo; b < hi; b++) {
        const uint2 x = blk[b];
        sv += x.x; st += x.y;
    }
    uint32_t all_v, all_t;
    uint32_t ev = lzm_block_scan<LZM_SCAN_WG / 64>(sv, wsum_v, all_v);
    uint32_t et = lzm_block_scan<LZM_SCAN_WG / 64>(st, wsum_t, all_t);
    for (uint32_t b = lo; b < hi; b++) {
        const uint2 x = blk[b];
        blk[b] = make_uint2(ev, et);
        ev += x.x; et += x.y;
    }
    if (threadIdx.x == 0) { totals[0] = all_v; totals[1] = all_t; }
}

__global__ void __launch_bounds__(LZM_TILE)
lz_k_mc_emit(const float* __restrict__ u, LzmGeom g, float thr, const uint16_t* __restrict__ info, const uint2* __restrict__ blk,
             const uint2* __restrict__ aux, uint32_t V_cap, uint32_t T_cap, float* __restrict__ vertices, int32_t* __restrict__ triangles) {
    __shared__ __attribute__((aligned(16))) uint8_t tl[256 * 16];
    __shared__ uint8_t sb[LZM_TILE + 1];
    __shared__ uint32_t wsum[LZM_TILE / 64];
    reinterpret_cast<uint4*>(tl)[threadIdx.x] = reinterpret_cast<const uint4*>(&lz_mc_tri[0][0])[threadIdx.x];   // 256 rows of 16 bytes
    LzmNode nd;
    lzm_node(u, g, thr, tl, 16, 15, sb, wsum, nd);
    if ((nd.cut | nd.ntri) == 0) return;      // (no barrier behind this point)
    uint2 base = blk[blockIdx.x];
    {
        const uint2 grp = aux[blockIdx.x / LZM_SCAN_WG];
        base.x += grp.x; base.y += grp.y;
    }
    if (nd.cut) {
        const uint32_t i = nd.row / g.Ry, j = nd.row - i * g.Ry;
        const float p[3] = {(float)i, (float)j, (float)nd.k};
        uint32_t vid = base.x + nd.local_v;
#pragma unroll
        for (int a = 0; a < 3; a++) {
            if (!(nd.cut >> a & 1u)) continue;
            const float u_hi = a == 0 ? nd.v10 : (a == 1 ? nd.v01 : u[nd.n + 1]);
            float t = (thr - nd.v00) / (u_hi - nd.v00);
            if (!(t >= 0.0f)) t = 0.0f;
            if (t > 1.0f) t = 1.0f;
            if (vid < V_cap) {
                float* o = vertices + (size_t)vid * 3;
                o[0] = a == 0 ? p[0] + t : p[0];
                o[1] = a == 1 ? p[1] + t : p[1];
                o[2] = a == 2 ? p[2] + t : p[2];
            }
            vid++;
        }
    }
    for (uint32_t r = 0; r < nd.ntri; r++) {
        const uint32_t tri = base.y + nd.local_t + r;
        if (tri >= T_cap) break;
        int32_t* o = triangles + (size_t)tri * 3;
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const uint32_t e = tl[nd.kase * 16 + 3 * r + c];
            const uint32_t a = e >> 2, p = e >> 1 & 1u, q = e & 1u;
            const uint32_t dx = a == 0 ? 0u : p, dy = a == 0 ? p : (a == 1 ? 0u : q), dz = a == 2 ? 0u : q;
            const uint32_t m = nd.n + dx * nd.sx + dy * nd.sy + dz;                                   // the node that owns the edge
            const uint32_t mb = (nd.row + dx * g.Ry + dy) * g.tiles + (nd.k + dz) / LZM_TILE;         // and its tile
            const uint32_t w = info[m];
            o[c] = (int32_t)(blk[mb].x + aux[mb / LZM_SCAN_WG].x + (w >> 3) + (uint32_t)__popc(w & ((1u << a) - 1u)));
        }
    }
}

// ---- host ----
static inline size_t lzm_align16(size_t v) { return (v + 15) & ~(size_t)15; }

static inline bool lzm_empty(uint32_t Rx, uint32_t Ry, uint32_t Rz) { return Rx < 2 || Ry < 2 || Rz < 2; }

// the lattice's geometry and tile count, or an error for a lattice beyond the 32-bit vertex keys 3 n + a
static int lzm_geom(uint32_t Rx, uint32_t Ry, uint32_t Rz, LzmGeom& g, uint32_t& nb, const char* who) {
    const uint64_t plane = (uint64_t)Rx * Ry;
    LZ_REQUIRE(plane < (1ull << 31) && 3 * plane * Rz < (1ull << 31), LZ_ERR_BAD_ARGUMENT, "%s: the lattice must have 3 Rx Ry Rz < 2^31", who);
    g.Rx = Rx; g.Ry = Ry; g.Rz = Rz;
    g.tiles = lz_div_up(Rz, LZM_TILE);
    nb = (uint32_t)(plane * g.tiles);
    return LZ_OK;
}

// workspace: tile totals uint2[nb] | group sums uint2[ceil(nb / LZM_SCAN_WG)] | node words uint16[Rx Ry Rz], each 16-byte aligned
static inline size_t lzm_ws_aux(uint32_t nb) { return lzm_align16((size_t)nb * sizeof(uint2)); }
static inline size_t lzm_ws_info(uint32_t nb) { return lzm_ws_aux(nb) + lzm_align16((size_t)lz_div_up(nb, LZM_SCAN_WG) * sizeof(uint2)); }

extern "C" size_t lz_mc_workspace(uint32_t Rx, uint32_t Ry, uint32_t Rz) {
    if (lzm_empty(Rx, Ry, Rz)) return 0;
    LzmGeom g;
    uint32_t nb;
    if (lzm_geom(Rx, Ry, Rz, g, nb, "mc_workspace") != LZ_OK) return 0;
    return lzm_ws_info(nb) + lzm_align16((size_t)Rx * Ry * Rz * sizeof(uint16_t));
}

extern "C" int lz_mc_count(const float* u, uint32_t Rx, uint32_t Ry, uint32_t Rz, float thr, void* workspace, uint32_t* totals, lz_stream_t stream) {
    if (lzm_empty(Rx, Ry, Rz)) return LZ_OK;
    LZ_REQUIRE(u && workspace && totals, LZ_ERR_BAD_ARGUMENT, "mc_count: null tensor");
    LZ_REQUIRE(((uintptr_t)workspace & 15) == 0, LZ_ERR_BAD_ARGUMENT, "mc_count: workspace must be 16-byte aligned");
    LzmGeom g;
    uint32_t nb;
    const int rc = lzm_geom(Rx, Ry, Rz, g, nb, "mc_count");
    if (rc != LZ_OK) return rc;
    uint2* blk = reinterpret_cast<uint2*>(workspace);
    uint2* aux = reinterpret_cast<uint2*>(reinterpret_cast<char*>(workspace) + lzm_ws_aux(nb));
    uint16_t* info = reinterpret_cast<uint16_t*>(reinterpret_cast<char*>(workspace) + lzm_ws_info(nb));
    const uint32_t na = lz_div_up(nb, LZM_SCAN_WG);
    hipLaunchKernelGGL(lz_k_mc_count, dim3(nb), dim3(LZM_TILE), 0, lz_st(stream), u, g, thr, info, blk);
    LZ_CHECK_LAUNCH("mc_count");
    hipLaunchKernelGGL(lz_k_mc_scan_tiles, dim3(na), dim3(LZM_SCAN_WG), 0, lz_st(stream), blk, nb, aux);
    LZ_CHECK_LAUNCH("mc_count (tile scan)");
    hipLaunchKernelGGL(lz_k_mc_scan, dim3(1), dim3(LZM_SCAN_WG), 0, lz_st(stream), aux, na, totals);
    LZ_CHECK_LAUNCH("mc_count (scan)");
    return LZ_OK;
}

extern "C" int lz_mc_emit(const float* u, uint32_t Rx, uint32_t Ry, uint32_t Rz, float thr, const void* workspace, uint32_t V_cap, uint32_t T_cap,
                          float* vertices, int32_t* triangles, lz_stream_t stream) {
    if (lzm_empty(Rx, Ry, Rz) || (V_cap == 0 && T_cap == 0)) return LZ_OK;
    LZ_REQUIRE(u && workspace && (V_cap == 0 || vertices) && (T_cap == 0 || triangles), LZ_ERR_BAD_ARGUMENT, "mc_emit: null tensor");
    LZ_REQUIRE(((uintptr_t)workspace & 15) == 0, LZ_ERR_BAD_ARGUMENT, "mc_emit: workspace must be 16-byte aligned");
    LzmGeom g;
    uint32_t nb;
    const int rc = lzm_geom(Rx, Ry, Rz, g, nb, "mc_emit");
    if (rc != LZ_OK) return rc;
    const uint2* blk = reinterpret_cast<const uint2*>(workspace);
    const uint2* aux = reinterpret_cast<const uint2*>(reinterpret_cast<const char*>(workspace) + lzm_ws_aux(nb));
    const uint16_t* info = reinterpret_cast<const uint16_t*>(reinterpret_cast<const char*>(workspace) + lzm_ws_info(nb));
    hipLaunchKernelGGL(lz_k_mc_emit, dim3(nb), dim3(LZM_TILE), 0, lz_st(stream), u, g, thr, info, blk, aux, V_cap, T_cap, vertices, triangles);
    LZ_CHECK_LAUNCH("mc_emit");
    return LZ_OK;
}
