// gms_census.hip -- the census of a gms_slam's particle maps (gridmapslam.h "census of the particles' maps"): per cell how many of a
// filter's particles hold it free and how many occupied, the majority map of those counts, its totals, and every particle's class
// matrix against that map.  Kernels and their launchers; the C-ABI is gms_slam_host.hip's, next to gms_slam_combined.  Integers
// throughout: every output is unique whatever the scheduling.  Nothing here is on the scan step's path.
//
//   the counting pass    grid (ceil(cells / GMS_CENSUS_TILE), ceil(n / GMS_CENSUS_CHUNK)), 256 lanes: a workgroup takes a tile of 512
//                        consecutive cells and a chunk of 32 particles, a lane the same pair of cells in every particle of the chunk --
//                        one 16-byte load per particle where the pair is 16-byte aligned (always, on an even cell count), two 8-byte
//                        loads where it is not (every other particle of an odd cell count), one where the last cell has no partner.
//                        Two compares per cell, `free | occupied << 16` summed in a register, one atomicAdd per non-zero cell word into
//                        the zeroed field: n <= 65535 keeps either half from carrying, integer sums make the split immaterial.  The
//                        split over particles is what fills the chip: 120^2 cells are 29 tiles.
//   the consensus pass   a lane per cell of the count field, workgroups striding over it: the class by the rule, a byte and -- WRITE_MAP
//                        -- a double stored, four ballots and a butterfly per wavefront, the four wavefronts' sums combined through LDS,
//                        one integer atomic per non-zero counter and workgroup (as k_warp counts).
//   the agreement pass   grid (ceil(cells / GMS_CENSUS_AGREE), n), 256 lanes: a workgroup takes a particle and 4096 cells, reads them
//                        as the counting pass does against the consensus bytes, nine ballots per cell of the pair, one atomic per
//                        non-zero counter and workgroup into the particle's record.
#include "gms_internal.h"
#include "gms_slam_device.h"

// the packed class word of one value: free in the low half, occupied in the high half, unknown (0, -0.0, NaN) nothing
__device__ __forceinline__ uint32_t census_word(double l) { return (l < 0.0 ? 1u : 0u) | (l > 0.0 ? 0x10000u : 0u); }
__device__ __forceinline__ int32_t census_class(double l) { return l > 0.0 ? 2 : l < 0.0 ? 1 : 0; }

// cells c and c + 1 (c even) of one particle's map: a 16-byte load where the pair's address allows it.  has1: the map holds c + 1
// (what it does not hold reads as 0.0, unknown).  The branches are uniform per wavefront except the tile's last pair.
__device__ __forceinline__ void census_pair(const double *__restrict__ map, int64_t c, bool has0, bool has1, double &a, double &b) {
    a = 0.0; b = 0.0;
    const double *q = map + c;
    if (has1) {
        if ((reinterpret_cast<uintptr_t>(q) & 15) == 0) {
            const double2 v = *reinterpret_cast<const double2 *>(q);
            a = v.x; b = v.y;
        } else {
            a = q[0]; b = q[1];
        }
    } else if (has0) {
        a = q[0];
    }
}

__global__ void __launch_bounds__(256)
k_census_count(SlamBufs sb, int32_t filter, int64_t cells, uint32_t *__restrict__ field) {
    const int32_t p0 = filter * sb.n_per;
    const int32_t k0 = (int32_t)blockIdx.y * GMS_CENSUS_CHUNK;                          // the chunk, filter-local
    const int32_t k1 = min(k0 + GMS_CENSUS_CHUNK, sb.n_per);
    const double *__restrict__ log = sb_log(sb, sb_epoch(sb, p0)[0] & 1) + (size_t)p0 * (size_t)cells;
    const int64_t c = (int64_t)blockIdx.x * GMS_CENSUS_TILE + 2 * (int64_t)threadIdx.x;
    const bool has0 = c < cells, has1 = c + 1 < cells;
    uint32_t w0 = 0u, w1 = 0u;
    if (!(cells & 1)) {                                                                 // every pair of every particle is aligned and whole
        if (has1) {
            const double2 *__restrict__ q = reinterpret_cast<const double2 *>(log + (size_t)k0 * (size_t)cells + c);
            const size_t pitch = (size_t)cells / 2;
#pragma unroll 8
            for (int32_t k = k0; k < k1; k++, q += pitch) {
                const double2 v = *q;
                w0 += census_word(v.x);
                w1 += census_word(v.y);
            }
        }
    } else {
        for (int32_t k = k0; k < k1; k++) {
            double a, b;
            census_pair(log + (size_t)k * (size_t)cells, c, has0, has1, a, b);
            w0 += census_word(a);
            w1 += census_word(b);
        }
    }
    if (w0) atomicAdd(field + c, w0);                                                   // (w0 != 0 implies has0, w1 != 0 implies has1)
    if (w1) atomicAdd(field + c + 1, w1);
}

// the consensus class of a count word under min_known: a tie goes to the obstacle
__device__ __forceinline__ int32_t census_consensus(uint32_t fr, uint32_t oc, uint32_t min_known) {
    return fr + oc < min_known ? 0 : oc >= fr ? 2 : 1;
}

__global__ void __launch_bounds__(256)
k_census_consensus(const uint32_t *__restrict__ field, int64_t cells, int32_t n, int32_t min_known, uint8_t *__restrict__ consensus, double *__restrict__ log_out,
                   gms_census_totals *__restrict__ totals) {
    __shared__ unsigned long long s_cnt[4][5];
    const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t cnt[4] = {0u, 0u, 0u, 0u};                                                 // cls[0..2], contested: wave-uniform
    unsigned long long minority = 0ull;                                                 // per lane
    for (int64_t base = (int64_t)blockIdx.x * 256; base < cells; base += (int64_t)gridDim.x * 256) {
        const int64_t c = base + threadIdx.x;
        const bool valid = c < cells;
        const uint32_t w = valid ? field[c] : 0u;
        const uint32_t fr = w & 0xFFFFu, oc = w >> 16;
        const int32_t cls = census_consensus(fr, oc, (uint32_t)min_known);
        if (valid) {
            if (consensus) consensus[c] = (uint8_t)cls;
            if (log_out) log_out[c] = cls == 2 ? 1.0 : cls == 1 ? -1.0 : 0.0;
        }
        if (totals) {
#pragma unroll
            for (int32_t k = 0; k < 3; k++) cnt[k] += (uint32_t)__popcll(__ballot(valid && cls == k));
            cnt[3] += (uint32_t)__popcll(__ballot(fr > 0u && oc > 0u));
            minority += fr < oc ? fr : oc;
        }
    }
    if (!totals) return;                                                                // (uniform per launch)
    for (int32_t o = 32; o; o >>= 1) minority += __shfl_xor(minority, o);
    if (lane == 0) {
#pragma unroll
        for (int32_t k = 0; k < 4; k++) s_cnt[wave][k] = cnt[k];
        s_cnt[wave][4] = minority;
    }
    __syncthreads();
    if (threadIdx.x < 5) {
        const unsigned long long sum = s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
        if (threadIdx.x < 3) { if (sum) atomicAdd(&totals->cls[threadIdx.x], (uint32_t)sum); }
        else if (threadIdx.x == 3) { if (sum) atomicAdd(&totals->contested, (uint32_t)sum); }
        else if (sum) atomicAdd(reinterpret_cast<unsigned long long *>(&totals->minority), sum);
    }
    if (blockIdx.x == 0 && threadIdx.x == 5) { totals->n = (uint32_t)n; totals->min_known = (uint32_t)min_known; }
}
static_assert(sizeof(gms_census_totals) == 32 && sizeof(unsigned long long) == sizeof(uint64_t), "k_census_consensus adds into the record's words");

__global__ void __launch_bounds__(256)
k_census_agree(SlamBufs sb, int32_t filter, int64_t cells, const uint8_t *__restrict__ consensus, uint32_t *__restrict__ agree) {
    __shared__ uint32_t s_cnt[4][9];
    const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int32_t p0 = filter * sb.n_per, k = blockIdx.y;                               // the particle, filter-local
    const double *__restrict__ map = sb_log(sb, sb_epoch(sb, p0)[0] & 1) + (size_t)(p0 + k) * (size_t)cells;
    const int64_t first = (int64_t)blockIdx.x * GMS_CENSUS_AGREE;
    uint32_t cnt[9] = {0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u, 0u};
    for (int32_t it = 0; it < GMS_CENSUS_AGREE / 512; it++) {
        const int64_t c = first + (int64_t)it * 512 + 2 * (int64_t)threadIdx.x;
        if (first + (int64_t)it * 512 >= cells) break;                                  // (uniform per workgroup)
        const bool has0 = c < cells, has1 = c + 1 < cells;
        double a, b;
        census_pair(map, c, has0, has1, a, b);
        const int32_t pa = census_class(a), pb = census_class(b);
        const int32_t ca = has0 ? consensus[c] : 0, cb = has1 ? consensus[c + 1] : 0;
#pragma unroll
        for (int32_t j = 0; j < 9; j++)
            cnt[j] += (uint32_t)__popcll(__ballot(has0 && pa == j / 3 && ca == j % 3)) + (uint32_t)__popcll(__ballot(has1 && pb == j / 3 && cb == j % 3));
    }
    if (lane == 0) {
#pragma unroll
        for (int32_t j = 0; j < 9; j++) s_cnt[wave][j] = cnt[j];
    }
    __syncthreads();
    if (threadIdx.x < 9) {
        const uint32_t sum = s_cnt[0][threadIdx.x] + s_cnt[1][threadIdx.x] + s_cnt[2][threadIdx.x] + s_cnt[3][threadIdx.x];
        if (sum) atomicAdd(agree + (size_t)k * 10 + threadIdx.x, sum);
    }
}

// ---- launchers (the entry point checks hipGetLastError) ---------------------------------------------------------------------------
void gms_launch_census_count(gms_map *m, const SlamBufs &sb, int32_t filter, uint32_t *d_field) {
    const int64_t cells = m->gd.cells;
    const dim3 grid((unsigned)((cells + GMS_CENSUS_TILE - 1) / GMS_CENSUS_TILE), (unsigned)((sb.n_per + GMS_CENSUS_CHUNK - 1) / GMS_CENSUS_CHUNK));
    gms_launch<k_census_count>(m, grid, dim3(256), 0, sb, filter, cells, d_field);
}
void gms_launch_census_consensus(gms_map *m, const uint32_t *d_field, int32_t n, int32_t min_known, uint8_t *d_consensus, double *d_log, gms_census_totals *d_totals) {
    const int64_t cells = m->gd.cells;
    gms_launch<k_census_consensus>(m, dim3(gms_grid(cells, 256, 1024)), dim3(256), 0, d_field, cells, n, min_known, d_consensus, d_log, d_totals);
}
void gms_launch_census_agree(gms_map *m, const SlamBufs &sb, int32_t filter, const uint8_t *d_consensus, uint32_t *d_agree) {
    const int64_t cells = m->gd.cells;
    const dim3 grid((unsigned)((cells + GMS_CENSUS_AGREE - 1) / GMS_CENSUS_AGREE), (unsigned)sb.n_per);
    gms_launch<k_census_agree>(m, grid, dim3(256), 0, sb, filter, cells, d_consensus, d_agree);
}
