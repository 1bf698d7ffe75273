// gms_modes.hip -- pose modes (gridmapslam.h "pose modes"): the particles of one shared-map filter binned in (x, y, theta), the occupied
// bins grouped into maximal 26-connected sets with the heading wrapping, and per set its anchor, count, box, strongest member and the
// weighted sums a pose estimate and its covariance are made of.  The integers are unique however the unions and the atomics are
// scheduled; the floating-point sums have ONE order (256 strided partials, then those in ascending order), so they are unique too.
//
// A translation unit of its own, kernels and C-ABI, on the query base (HostStage) beside gms_scatter.hip: no kernel of the other units
// is compiled differently for it.
//
//   k_modes_clear       a lane per bin: count 0, label = own index; the three counters cleared.
//   k_modes_bin         (1) a lane per particle: its bin (gms_map_clearance_poses' cell rule, the heading from one double multiply and a
//                       floor) stored, the bin's count raised -- the lanes of a wavefront that share a bin combined first (wave_each_key), ONE atomic
//                       per distinct bin -- and the OUTSIDE particles counted, one atomic per wavefront.
//   k_modes_unite       (2) a lane per bin: an occupied bin is united with its 13 forward neighbours -- 4 in its own heading layer, the
//                       9 of layer bt + 1 mod n_theta -- in the global label field (region_unite, gms_regions.h: the larger root
//                       always under the smaller, so the final root is the anchor).  n_theta == 2 meets every
//                       cross-layer pair from both sides, which a union does not mind; n_theta == 1 has no other layer.
//   k_modes_flatten     (3) every occupied bin chases to its root and stores it; "I am my own root" is the bin's flag.
//   gms_launch_scan     the exclusive scan of the flags (gms_query.hip): the roots in linear order = the modes in anchor order; the
//                       total is the number of modes.
//   k_modes_table_init, k_modes_reduce, k_modes_finish
//                       (4) the table: a wavefront per 64 bins looks up every occupied bin's mode, and the lanes that share one combine
//                       (wave_each_key; count, bins, box: butterflies over the group) before ONE lane issues the atomics -- integer
//                       min / max / add only.  The finish flags count >= min_count; the scan again, then k_modes_emit stores the kept modes'
//                       integers in order, the first `cap` of them, and each stored record's anchor index for step 6.
//   k_modes_labels      (5) a lane per particle: the root of its bin, or GMS_MODE_NONE.
//   k_modes_sums        (6) one workgroup of 256 lanes per STORED record: lane l walks the particles l, l + 256, ... in ascending order
//                       (eight labels loaded ahead at a time; the adds stay in order), its eight partial sums and its strongest member
//                       in registers; the partials go to LDS (rows padded by one double: the eight lanes that add a row each hit eight
//                       banks), and lane k < 8 adds sum k's 256 partials in ascending order, lane 8 picks the strongest.
//
// No workgroup waits on another.  A mode holds at least one particle and one bin, so min(n, bins) rows of the table always suffice:
// nothing is sized from a read-back, and the ONE wait on the stream is for *n_found, *n_outside and the host form's copies.
#undef GMS_STAMPS
#include <limits.h>
#include <stddef.h>
#include <stdlib.h>

#include <algorithm>

#include "gms_regions.h"

#define MOD_NT 256
#define MOD_NONE 0xffffffffu
#define MOD_MAX_BINS ((int64_t)1 << 22)
#define MOD_AHEAD 8                      // labels k_modes_sums loads ahead of its adds

static_assert(GMS_MODE_NONE == MOD_NONE, "the header's constant is the kernels'");
static_assert(sizeof(gms_modes) == 16 && sizeof(gms_mode) == 112 && offsetof(gms_mode, count) == 12 && offsetof(gms_mode, bins) == 16 &&
              offsetof(gms_mode, strongest) == 20 && offsetof(gms_mode, min_bx) == 24 && offsetof(gms_mode, pad) == 40 && offsetof(gms_mode, w) == 48 &&
              offsetof(gms_mode, wyy) == 104, "the header fixes the record's offsets");

// a mode's integers as the table keeps them: the first 40 bytes of a gms_mode
struct ModeRow {
    int32_t anchor_bx, anchor_by, anchor_bt, count, bins, strongest, min_bx, min_by, max_bx, max_by;
};
static_assert(sizeof(ModeRow) == offsetof(gms_mode, pad), "a row is a record's head");

// the request as the kernels see it
struct ModesDev {
    int32_t bin_cells, n_theta, BW, BH, NB;
    double k;                            // (double)n_theta * 0.15915494309189535, rounded once on the host
};

__global__ void __launch_bounds__(MOD_NT)
k_modes_clear(uint32_t *__restrict__ cnt, uint32_t *__restrict__ lab, int32_t NB, uint32_t *__restrict__ ctl) {
    const int32_t b = (int32_t)blockIdx.x * MOD_NT + (int32_t)threadIdx.x;
    if (b < 4) ctl[b] = 0u;
    if (b >= NB) return;
    cnt[b] = 0u;
    lab[b] = (uint32_t)b;
}

// pose: ONE map's particles [n][3]; pbin [n]; ctl[2]: the OUTSIDE particles
__global__ void __launch_bounds__(MOD_NT)
k_modes_bin(GridDev g, ModesDev q, const float *__restrict__ pose, int32_t n, uint32_t *__restrict__ pbin, uint32_t *__restrict__ cnt, uint32_t *__restrict__ ctl) {
    const int32_t i = (int32_t)blockIdx.x * MOD_NT + (int32_t)threadIdx.x, lane = (int32_t)threadIdx.x & 63;
    uint32_t bin = MOD_NONE;
    if (i < n) {
        const int32_t gx = j_cell_exact((double)pose[3 * (size_t)i] - g.posx, g.res);             // GridMap.java:273
        const int32_t gy = j_cell_exact((double)pose[3 * (size_t)i + 1] - g.posy, g.res);         // :274
        const double f = floor((double)pose[3 * (size_t)i + 2] * q.k);
        if (!(gx < 0 || gy < 0 || gx >= g.W || gy >= g.H) && fabs(f) < 2147483648.0) {            // (a NaN f compares false: OUTSIDE)
            int32_t bt = (int32_t)f % q.n_theta;
            if (bt < 0) bt += q.n_theta;
            bin = (uint32_t)((bt * q.BH + gy / q.bin_cells) * q.BW + gx / q.bin_cells);
        }
        pbin[i] = bin;
    }
    const uint64_t out = __ballot(i < n && bin == MOD_NONE);
    if (lane == 0 && out) atomicAdd(ctl + 2, (uint32_t)__popcll(out));
    wave_each_key(bin, MOD_NONE, [&](uint32_t B, bool, uint64_t grp, bool leader) {
        if (leader) atomicAdd(cnt + B, (uint32_t)__popcll(grp));
    });
}

__global__ void __launch_bounds__(MOD_NT)
k_modes_unite(ModesDev q, const uint32_t *__restrict__ cnt, uint32_t *lab) {
    const int32_t b = (int32_t)blockIdx.x * MOD_NT + (int32_t)threadIdx.x;
    if (b >= q.NB || cnt[b] == 0u) return;
    const int32_t bx = b % q.BW, by = (b / q.BW) % q.BH, bt = b / (q.BW * q.BH);
    auto join = [&](int32_t ox, int32_t oy, int32_t ot) {
        if (ox < 0 || ox >= q.BW || oy < 0 || oy >= q.BH) return;
        const int32_t o = (ot * q.BH + oy) * q.BW + ox;
        if (cnt[o] != 0u) region_unite(lab, (uint32_t)b, (uint32_t)o);
    };
    join(bx + 1, by, bt);
    for (int32_t dx = -1; dx <= 1; dx++) join(bx + dx, by + 1, bt);
    if (q.n_theta == 1) return;
    const int32_t ot = bt + 1 == q.n_theta ? 0 : bt + 1;
    for (int32_t dy = -1; dy <= 1; dy++)
        for (int32_t dx = -1; dx <= 1; dx++) join(bx + dx, by + dy, ot);
}

// flag [NB]: 1 for a root, 0 elsewhere
__global__ void __launch_bounds__(MOD_NT)
k_modes_flatten(const uint32_t *__restrict__ cnt, uint32_t *lab, int32_t NB, uint32_t *__restrict__ flag) {
    const int32_t b = (int32_t)blockIdx.x * MOD_NT + (int32_t)threadIdx.x;
    if (b >= NB) return;
    uint32_t root = 0u;
    if (cnt[b] != 0u) {
        const uint32_t r = region_find(lab, (uint32_t)b);
        if (r != (uint32_t)b) __atomic_store_n(lab + b, r, __ATOMIC_RELAXED);   // (another lane's chase reads the old parent or the root: both lead there)
        root = r == (uint32_t)b ? 1u : 0u;
    }
    flag[b] = root;
}

// the first min(ctl[0], tcap) rows
__global__ void __launch_bounds__(MOD_NT)
k_modes_table_init(ModeRow *__restrict__ row, const uint32_t *__restrict__ ctl, int32_t tcap) {
    const int32_t n = (int32_t)std::min<uint32_t>(ctl[0], (uint32_t)tcap);
    for (int32_t i = (int32_t)blockIdx.x * MOD_NT + (int32_t)threadIdx.x; i < n; i += (int32_t)gridDim.x * MOD_NT)
        row[i] = ModeRow{0, 0, 0, 0, 0, -1, INT_MAX, INT_MAX, -1, -1};
}

// a wavefront per 64 bins.  num / nblk: the scan of the root flags; modes behind tcap are left out (there are none: see the head)
__global__ void __launch_bounds__(MOD_NT)
k_modes_reduce(ModesDev q, const uint32_t *__restrict__ cnt, const uint32_t *__restrict__ lab, const uint32_t *__restrict__ num, const uint32_t *__restrict__ nblk,
               ModeRow *row, int32_t tcap) {
    const int32_t b = (int32_t)blockIdx.x * MOD_NT + (int32_t)threadIdx.x;
    const int32_t c = b < q.NB ? (int32_t)cnt[b] : 0;
    uint32_t mode = MOD_NONE;
    int32_t bx = 0, by = 0;
    if (c != 0) {
        const uint32_t r = lab[b];
        bx = b % q.BW;
        by = (b / q.BW) % q.BH;
        mode = scan_prefix(num, nblk, r);
        if (mode >= (uint32_t)tcap) mode = MOD_NONE;
        else if (r == (uint32_t)b) { row[mode].anchor_bx = bx; row[mode].anchor_by = by; row[mode].anchor_bt = b / (q.BW * q.BH); }   // (the root alone writes these)
    }
    wave_each_key(mode, MOD_NONE, [&](uint32_t R, bool in, uint64_t grp, bool leader) {
        const int32_t members = wave_add(in ? c : 0);
        const int32_t lo_x = wave_min(in ? bx : INT_MAX), lo_y = wave_min(in ? by : INT_MAX);
        const int32_t hi_x = wave_max(in ? bx : -1), hi_y = wave_max(in ? by : -1);
        if (!leader) return;
        ModeRow *m = row + R;
        atomicAdd(&m->count, members);
        atomicAdd(&m->bins, (int32_t)__popcll(grp));
        atomicMin(&m->min_bx, lo_x);
        atomicMin(&m->min_by, lo_y);
        atomicMax(&m->max_bx, hi_x);
        atomicMax(&m->max_by, hi_y);
    });
}

// kept [i] = count >= min_count
__global__ void __launch_bounds__(MOD_NT)
k_modes_finish(const ModeRow *__restrict__ row, const uint32_t *__restrict__ ctl, int32_t tcap, int32_t min_count, uint32_t *__restrict__ kept) {
    const int32_t n = (int32_t)std::min<uint32_t>(ctl[0], (uint32_t)tcap);
    for (int32_t i = (int32_t)blockIdx.x * MOD_NT + (int32_t)threadIdx.x; i < n; i += (int32_t)gridDim.x * MOD_NT) kept[i] = row[i].count >= min_count ? 1u : 0u;
}

// kept / kblocks: the scan of the flags; out [out_cap], anchors [out_cap]: every stored record's label
__global__ void __launch_bounds__(MOD_NT)
k_modes_emit(ModesDev q, const ModeRow *__restrict__ row, const uint32_t *__restrict__ kept, const uint32_t *__restrict__ kblocks, const uint32_t *__restrict__ ctl,
             int32_t tcap, int32_t min_count, gms_mode *__restrict__ out, uint32_t *__restrict__ anchors, int32_t out_cap) {
    const int32_t n = (int32_t)std::min<uint32_t>(ctl[0], (uint32_t)tcap);
    for (int32_t i = (int32_t)blockIdx.x * MOD_NT + (int32_t)threadIdx.x; i < n; i += (int32_t)gridDim.x * MOD_NT) {
        const ModeRow r = row[i];
        if (r.count < min_count) continue;
        const uint32_t at = scan_prefix(kept, kblocks, i);
        if (at >= (uint32_t)out_cap) continue;
        gms_mode *o = out + at;
        o->anchor_bx = r.anchor_bx; o->anchor_by = r.anchor_by; o->anchor_bt = r.anchor_bt;
        o->count = r.count; o->bins = r.bins;
        o->min_bx = r.min_bx; o->min_by = r.min_by; o->max_bx = r.max_bx; o->max_by = r.max_by;
        o->pad[0] = o->pad[1] = 0;
        anchors[at] = (uint32_t)((r.anchor_bt * q.BH + r.anchor_by) * q.BW + r.anchor_bx);
    }
}

// plab [n], out (may be NULL) [n]
__global__ void __launch_bounds__(MOD_NT)
k_modes_labels(const uint32_t *__restrict__ pbin, const uint32_t *__restrict__ lab, int32_t n, uint32_t *__restrict__ plab, uint32_t *__restrict__ out) {
    const int32_t i = (int32_t)blockIdx.x * MOD_NT + (int32_t)threadIdx.x;
    if (i >= n) return;
    const uint32_t b = pbin[i], l = b == MOD_NONE ? MOD_NONE : lab[b];
    plab[i] = l;
    if (out) out[i] = l;
}

// grid: the records that can be stored; workgroup r serves record r < min(ctl[1], cap).  pose, cs, wgt: ONE map's particles
__global__ void __launch_bounds__(MOD_NT)
k_modes_sums(const uint32_t *__restrict__ plab, int32_t n, const float *__restrict__ pose, const float *__restrict__ cs, const double *__restrict__ wgt,
             const uint32_t *__restrict__ anchors, const uint32_t *__restrict__ ctl, int32_t cap, gms_mode *__restrict__ out) {
    __shared__ double s_sum[8][MOD_NT + 1];
    __shared__ double s_bw[MOD_NT];
    __shared__ int32_t s_bi[MOD_NT];
    const int32_t rec = (int32_t)blockIdx.x, l = (int32_t)threadIdx.x;
    if ((uint32_t)rec >= std::min<uint32_t>(ctl[1], (uint32_t)cap)) return;     // (uniform)
    const uint32_t L = anchors[rec];
    double s[8] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    double best_w = 0.0;
    int32_t best_i = -1;
    for (int32_t base = l; base < n; base += MOD_AHEAD * MOD_NT) {
        uint32_t lb[MOD_AHEAD];
#pragma unroll
        for (int32_t u = 0; u < MOD_AHEAD; u++) {
            const int32_t i = base + u * MOD_NT;
            lb[u] = i < n ? plab[i] : MOD_NONE;
        }
#pragma unroll
        for (int32_t u = 0; u < MOD_AHEAD; u++) {
            if (lb[u] != L) continue;
            const int32_t i = base + u * MOD_NT;
            const double a = wgt[i], X = (double)pose[3 * (size_t)i], Y = (double)pose[3 * (size_t)i + 1];
            const double C = (double)cs[2 * (size_t)i], S = (double)cs[2 * (size_t)i + 1];
            s[0] += a;
            s[1] += a * X;
            s[2] += a * Y;
            s[3] += a * C;
            s[4] += a * S;
            s[5] += a * (X * X);                                                // (the product of two floats is exact in double)
            s[6] += a * (X * Y);
            s[7] += a * (Y * Y);
            if (a == a && (best_i < 0 || a > best_w)) { best_w = a; best_i = i; }
        }
    }
#pragma unroll
    for (int32_t k = 0; k < 8; k++) s_sum[k][l] = s[k];
    s_bw[l] = best_w;
    s_bi[l] = best_i;
    __syncthreads();
    gms_mode *o = out + rec;
    if (l < 8) {
        double t = s_sum[l][0];
        for (int32_t j = 1; j < MOD_NT; j++) t += s_sum[l][j];
        (&o->w)[l] = t;
    } else if (l == 8) {
        double bw = 0.0;
        int32_t bi = -1;
        for (int32_t j = 0; j < MOD_NT; j++) {
            const int32_t ij = s_bi[j];
            if (ij < 0) continue;
            const double wj = s_bw[j];
            if (bi < 0 || wj > bw || (wj == bw && ij < bi)) { bw = wj; bi = ij; }
        }
        o->strongest = bi;
    }
}

// ---- host ----------------------------------------------------------------------------------------------------------------------
struct ModesBins {                       // the bins' part of the scratch
    uint32_t *cnt, *lab, *num, *nblk;
};
static inline ModesBins modes_bins(const gms_pf *pf) {
    ModesBins b;
    const size_t cap = (size_t)pf->modes.bins_cap;
    b.cnt = pf->modes.d_bins; b.lab = b.cnt + cap; b.num = b.lab + cap; b.nblk = b.num + cap;
    return b;
}
struct ModesTable {
    ModeRow *row;
    uint32_t *kept, *kblocks, *anchors;
};
static inline ModesTable modes_table(const gms_pf *pf) {
    ModesTable t;
    const size_t cap = (size_t)pf->modes.table_cap;
    t.row = reinterpret_cast<ModeRow *>(pf->modes.d_table);
    t.kept = reinterpret_cast<uint32_t *>(pf->modes.d_table + cap * sizeof(ModeRow));
    t.anchors = t.kept + cap;
    t.kblocks = t.anchors + cap;
    return t;
}
static int modes_buffers(gms_pf *pf, int64_t NB, int64_t rows) {
    auto &s = pf->modes;
    int rc = gms_dev_alloc(&s.d_part, 2 * (size_t)pf->n * sizeof(uint32_t), "gms_pf_modes", "the particles' bins and labels");
    if (!rc) rc = gms_dev_alloc(&s.d_ctl, 4 * sizeof(uint32_t), "gms_pf_modes", "the counters");
    const hipStream_t *st = &pf->map->stream;                                   // (both grow behind a wait on it and never shrink)
    if (!rc) rc = gms_dev_grow(&s.d_bins, &s.bins_cap, NB, GMS_SCAN, st, [](size_t c) { return (3 * c + c / GMS_SCAN + 1) * sizeof(uint32_t); }, "gms_pf_modes", "the bin counts, the label field and its scan");
    if (!rc) rc = gms_dev_grow(&s.d_table, &s.table_cap, rows, GMS_SCAN, st, [](size_t c) { return c * (sizeof(ModeRow) + 2 * sizeof(uint32_t)) + (c / GMS_SCAN + 1) * sizeof(uint32_t); }, "gms_pf_modes", "the mode table");
    if (!rc) rc = gms_pinned_alloc(&s.h_ctl, 4 * sizeof(uint32_t), "gms_pf_modes");
    return rc;
}

static int pf_modes(gms_pf *pf, int32_t mi, const gms_modes *q, uint32_t *labels, gms_mode *records, int32_t cap, int32_t *n_found, int32_t *n_outside,
                    bool on_device) {
    const char *what = on_device ? "gms_pf_modes_dev" : "gms_pf_modes";
    if (!pf || !q) return gms_fail(GMS_ERR_INVALID, "%s: null argument (the filter and the request are required)", what);
    int rc = gms_modes_check(q);
    if (rc) return rc;
    if (pf->slam_owned) return gms_fail(GMS_ERR_STATE, "%s: this filter's particles own maps (gms_slam): there is no one map to bin them in", what);
    if (pf_is_shard(pf)) return gms_fail(GMS_ERR_STATE, "%s: a shard of a filter: its modes span the ranks, and the bin counts are not exchanged", what);
    gms_map *m = pf->map;
    if (mi < 0 || mi >= pf->n_maps) return gms_fail(GMS_ERR_INVALID, "%s: map index out of range", what);
    if (cap < 0 || (cap > 0 && !records) || (cap == 0 && records)) return gms_fail(GMS_ERR_INVALID, "%s: cap >= 0, and records exactly when cap > 0", what);
    const GridDev &g = m->gd;
    const int64_t BW = ((int64_t)g.W + q->bin_cells - 1) / q->bin_cells, BH = ((int64_t)g.H + q->bin_cells - 1) / q->bin_cells, NB = BW * BH * q->n_theta;
    if (NB > MOD_MAX_BINS) return gms_fail(GMS_ERR_INVALID, "%s: %lld x %lld x %d bins exceed 2^22", what, (long long)BW, (long long)BH, q->n_theta);
    if (on_device && ((uintptr_t)labels & 3 || (uintptr_t)records & 7))
        return gms_fail(GMS_ERR_INVALID, "%s: the labels must be 4-byte aligned, the records 8-byte aligned", what);
    HIPCHK(hipSetDevice(m->device));
    const int32_t n = pf->n, rows = (int32_t)std::min<int64_t>(n, NB), stored = std::min(cap, rows);
    rc = modes_buffers(pf, NB, rows);
    if (rc) return rc;
    HostStage st(m, on_device);
    const size_t label_bytes = labels ? (size_t)n * sizeof(uint32_t) : 0;
    const size_t p_labels = st.part(label_bytes), p_records = st.part((size_t)stored * sizeof(gms_mode));
    rc = st.open();
    if (rc) return rc;
    uint32_t *d_labels = labels ? st.at(p_labels, labels) : nullptr;
    gms_mode *d_records = cap > 0 ? st.at(p_records, records) : nullptr;
    gms_launch_pf_combine(pf);                                                  // the weights out of a pending scoring pass
    ModesDev d;
    d.bin_cells = q->bin_cells; d.n_theta = q->n_theta; d.BW = (int32_t)BW; d.BH = (int32_t)BH; d.NB = (int32_t)NB;
    d.k = (double)q->n_theta * 0.15915494309189535;
    const ModesBins b = modes_bins(pf);
    const ModesTable t = modes_table(pf);
    const int32_t tcap = (int32_t)pf->modes.table_cap;                         // (at most 2^20 + 1023)
    uint32_t *pbin = pf->modes.d_part, *plab = pbin + n, *ctl = pf->modes.d_ctl;
    const float *pose = pf->d_pose + 3 * (size_t)mi * (size_t)n, *cs = pf->d_cs + 2 * (size_t)mi * (size_t)n;
    const double *wgt = pf->d_w + (size_t)mi * (size_t)n;
    hipStream_t s = m->stream;
    const unsigned gb = (unsigned)((NB + MOD_NT - 1) / MOD_NT), gp = (unsigned)((n + MOD_NT - 1) / MOD_NT), gt = gms_grid(rows, MOD_NT, 1024);
    hipLaunchKernelGGL(k_modes_clear, dim3(gb), dim3(MOD_NT), 0, s, b.cnt, b.lab, d.NB, ctl);
    hipLaunchKernelGGL(k_modes_bin, dim3(gp), dim3(MOD_NT), 0, s, g, d, pose, n, pbin, b.cnt, ctl);
    hipLaunchKernelGGL(k_modes_unite, dim3(gb), dim3(MOD_NT), 0, s, d, b.cnt, b.lab);
    hipLaunchKernelGGL(k_modes_flatten, dim3(gb), dim3(MOD_NT), 0, s, b.cnt, b.lab, d.NB, b.num);
    gms_launch_scan(s, b.num, nullptr, NB, b.nblk, ctl);
    hipLaunchKernelGGL(k_modes_table_init, dim3(gt), dim3(MOD_NT), 0, s, t.row, ctl, tcap);
    hipLaunchKernelGGL(k_modes_reduce, dim3(gb), dim3(MOD_NT), 0, s, d, b.cnt, b.lab, b.num, b.nblk, t.row, tcap);
    hipLaunchKernelGGL(k_modes_finish, dim3(gt), dim3(MOD_NT), 0, s, t.row, ctl, tcap, q->min_count, t.kept);
    gms_launch_scan(s, t.kept, ctl, rows, t.kblocks, ctl + 1);                  // (the modes are min(n, bins) = rows at most)
    hipLaunchKernelGGL(k_modes_labels, dim3(gp), dim3(MOD_NT), 0, s, pbin, b.lab, n, plab, d_labels);
    if (stored > 0) {
        hipLaunchKernelGGL(k_modes_emit, dim3(gt), dim3(MOD_NT), 0, s, d, t.row, t.kept, t.kblocks, ctl, tcap, q->min_count, d_records, t.anchors, stored);
        hipLaunchKernelGGL(k_modes_sums, dim3((unsigned)stored), dim3(MOD_NT), 0, s, plab, n, pose, cs, wgt, t.anchors, ctl, stored, d_records);
    }
    HIPCHK(hipGetLastError());
    uint32_t *h = pf->modes.h_ctl;
    HIPCHK(hipMemcpyAsync(h, ctl, 4 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIPCHK(hipStreamSynchronize(s));
    if (n_found) *n_found = (int32_t)h[1];
    if (n_outside) *n_outside = (int32_t)h[2];
    st.fetch(labels, p_labels, label_bytes);
    st.fetch(records, p_records, (size_t)std::min<int64_t>(h[1], stored) * sizeof(gms_mode));
    return st.finish(nullptr);
}

extern "C" {

int gms_modes_check(const gms_modes *q) {
    REQUIRE(q, "gms_modes: null request");
    REQUIRE(q->bin_cells >= 1, "gms_modes: bin_cells must be at least 1");
    REQUIRE(q->n_theta >= 1 && q->n_theta <= 64, "gms_modes: 1 <= n_theta <= 64 heading bins");
    REQUIRE(q->min_count >= 1, "gms_modes: min_count must be at least 1");
    return GMS_OK;
}
int gms_pf_modes(gms_pf *pf, int32_t mi, const gms_modes *q, uint32_t *labels, gms_mode *records, int32_t cap, int32_t *n_found, int32_t *n_outside) {
    return pf_modes(pf, mi, q, labels, records, cap, n_found, n_outside, false);
}
int gms_pf_modes_dev(gms_pf *pf, int32_t mi, const gms_modes *q, uint32_t *dev_labels, gms_mode *dev_records, int32_t cap, int32_t *n_found,
                     int32_t *n_outside) {
    return pf_modes(pf, mi, q, dev_labels, dev_records, cap, n_found, n_outside, true);
}

}  // extern "C"
