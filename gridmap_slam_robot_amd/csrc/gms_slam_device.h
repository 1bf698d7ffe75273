// gms_slam_device.h -- what the kernels of a gms_slam share across translation units (gms_pf_kernels.hip and gms_slam_kernels.hip in
// the device unit, gms_slam_align.hip and gms_slam_beams.hip on their own): the motion-model sample of one particle, the handle's
// buffers as a kernel addresses them, and the prologue of a kernel that takes one workgroup per particle -- slam_generation (the
// batch's filter, the maps' current generation) and slam_pose_draw (wavefront 0 draws the motion-model sample or reads the pose).
// All four such kernels take slam_generation.  k_slam_align and k_slam_beam_score take slam_pose_draw too; k_slam_particle and
// k_slam_refine, the two kernels the benchmark times, keep its lines written out: with the helper their instruction streams differ
// from the hand-written ones (operands commuted in the Philox rounds, other registers), and they change only where that is free.
#pragma once
#include "gms_device.h"

// Philox4x32-10 (the motion model's variates: gms_pf_kernels.hip "Odometry.apply for every particle")
__device__ __forceinline__ void philox_round(uint32_t c[4], const uint32_t k[2]) {
    const uint64_t p0 = (uint64_t)0xD2511F53u * c[0], p1 = (uint64_t)0xCD9E8D57u * c[2];
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c[1] ^ k[0], n1 = (uint32_t)p1;
    const uint32_t n2 = (uint32_t)(p0 >> 32) ^ c[3] ^ k[1], n3 = (uint32_t)p0;
    c[0] = n0; c[1] = n1; c[2] = n2; c[3] = n3;
}

// Odometry.apply for one particle, on values (J/slam/Odometry.java:77-96): (x, y, th) move on, (fc, fs) is the new heading's trig.
// index: the particle's global index (+ the map's counter offset); the variates are Philox4x32-10 on (index, sequence) keyed by seed.
struct MotionArgs {
    int32_t on;
    double d_center, d_theta, d_center_sd, d_theta_sd;
    uint64_t seed, sequence;
    int64_t index0;             // global index of the launch's particle 0 (a shard's offset): the variates are keyed by the GLOBAL index
};
// one odometry step as the kernels take it; motion NULL: no sample is drawn (on = 0)
static MotionArgs motion_args(const MotionModel *motion, int64_t index0) {
    MotionArgs mo;
    mo.on = 0; mo.d_center = mo.d_theta = mo.d_center_sd = mo.d_theta_sd = 0.0; mo.seed = mo.sequence = 0; mo.index0 = index0;
    if (motion) {
        mo.on = 1; mo.d_center = motion->d_center; mo.d_theta = motion->d_theta; mo.seed = motion->seed; mo.sequence = motion->sequence;
        motion_deviations(motion->d_center, motion->d_theta, &mo.d_center_sd, &mo.d_theta_sd);
    }
    return mo;
}
__device__ __forceinline__ void motion_apply(float &x, float &y, float &th, float &fc, float &fs, uint64_t index, double d_center,
                                             double d_theta, double d_center_sd, double d_theta_sd, uint64_t seed, uint64_t sequence) {
    uint32_t c[4] = { (uint32_t)index, (uint32_t)(index >> 32), (uint32_t)sequence, (uint32_t)(sequence >> 32) };
    uint32_t k[2] = { (uint32_t)seed, (uint32_t)(seed >> 32) };
#pragma unroll
    for (int r = 0; r < 10; r++) {
        philox_round(c, k);
        k[0] += 0x9E3779B9u; k[1] += 0xBB67AE85u;
    }
    const double u1 = ((double)(((uint64_t)(c[0] >> 5) << 26) | (uint64_t)(c[1] >> 6)) + 0.5) * (1.0 / 9007199254740992.0);
    const double u2 = ((double)(((uint64_t)(c[2] >> 5) << 26) | (uint64_t)(c[3] >> 6)) + 0.5) * (1.0 / 9007199254740992.0);
    const double rad = sqrt(-2.0 * log(u1));
    const double z0 = rad * cos(2.0 * 3.141592653589793 * u2), z1 = rad * sin(2.0 * 3.141592653589793 * u2);
    const double d = d_center + d_center_sd * z0;                                // ndCenter.sample()  :80
    const double theta = d_theta + d_theta_sd * z1;                              // ndTheta.sample()   :81
    th = (float)angle_constrain((double)th + theta);                             // :92
    pose_trig(th, fc, fs);                                                       // MathUtil.cos(float) :93
    x = (float)((double)x + (double)fc * d);                                     // :93  p.x += cos * d
    y = (float)((double)y + (double)fs * d);                                     // :94
}

// a generation's arrays out of SlamBufs by SELECTION, never by a run-time index into the by-value kernel argument (that moves the
// struct -- and whatever else the compiler then keeps addressable -- into scratch memory: k_slam_gather_one ran at a quarter of its speed)
__device__ __forceinline__ double *sb_log(const SlamBufs &sb, int32_t g) { return g ? sb.log[1] : sb.log[0]; }
__device__ __forceinline__ double *sb_lik(const SlamBufs &sb, int32_t g) { return g ? sb.lik[1] : sb.lik[0]; }
__device__ __forceinline__ uint32_t *sb_code(const SlamBufs &sb, int32_t g) { return g ? sb.code[1] : sb.code[0]; }
// the generation pair of particle p's filter: {draws that ran, the last resample() drew} (one filter: sb.epoch itself)
__device__ __forceinline__ const int32_t *sb_epoch(const SlamBufs &sb, int32_t p) { return sb.epoch + 2 * (p / sb.n_per); }
// a batched update: particle p's filter f = p / n -- its scan, count, motion and skipUpdate (SlamFilterArgs), its generation pair.
// The motion-model variates are keyed by the filter-local index (mo.index0 = -f n): what a stand-alone handle of that seed draws.
__device__ __forceinline__ void slam_batch_filter(const SlamBatch &bt, int32_t p, const gms_beam *__restrict__ &beams, int32_t &B, MotionArgs &mo,
                                                  int32_t &integrate, const int32_t *&epoch) {
    const int32_t f = p / bt.n;
    const SlamFilterArgs fa = bt.tab[f];
    beams += (size_t)f * (size_t)bt.beam_stride;
    B = fa.count;
    mo.on &= fa.flags & 1;
    mo.d_center = fa.d_center; mo.d_theta = fa.d_theta; mo.d_center_sd = fa.d_center_sd; mo.d_theta_sd = fa.d_theta_sd;
    mo.seed = fa.seed;
    mo.index0 = -(int64_t)f * bt.n;
    integrate &= (fa.flags >> 1) & 1;
    epoch += 2 * f;
}
// The first lines of a kernel that takes one workgroup per particle p: BATCH, the particle's filter first (slam_batch_filter: its scan,
// count, motion and generation pair; integrate: its skipUpdate, for the kernel that integrates); then the current generation of the
// particles' maps (SlamBufs)
template <bool BATCH>
__device__ __forceinline__ int32_t slam_generation(const SlamBufs &sb, const SlamBatch &bt, int32_t p, const gms_beam *__restrict__ &beams, int32_t &B,
                                                   MotionArgs &mo, int32_t &integrate) {
    const int32_t *epoch = sb.epoch;
    if constexpr (BATCH) slam_batch_filter(bt, p, beams, B, mo, integrate, epoch);
    return epoch[0] & 1;
}
template <bool BATCH>
__device__ __forceinline__ int32_t slam_generation(const SlamBufs &sb, const SlamBatch &bt, int32_t p, const gms_beam *__restrict__ &beams, int32_t &B, MotionArgs &mo) {
    int32_t integrate = 0;
    return slam_generation<BATCH>(sb, bt, p, beams, B, mo, integrate);
}
// Wavefront 0's part of it, every lane: sampleMotionModel (SLAM.java:90, Odometry.java:77-96) where the update asked for a sample and no
// launch in front drew it -- written back to pose / cs by lane 0 -- or the pose as it stands; lane 0 publishes x, y, theta into s_pose
// [0..2] and, TRIG, the heading's float trig into s_pose[3..4] (cs[] always matches pose[]: k_pose_trig).  The caller's barrier
// follows.  Returns theta
template <bool TRIG>
__device__ __forceinline__ float slam_pose_draw(const MotionArgs &mo, int32_t p, int32_t lane, float *pose, float *cs, float *s_pose) {
    float x = pose[3 * (size_t)p], y = pose[3 * (size_t)p + 1], th = pose[3 * (size_t)p + 2], c, sn;
    if (mo.on) motion_apply(x, y, th, c, sn, (uint64_t)(mo.index0 + p), mo.d_center, mo.d_theta, mo.d_center_sd, mo.d_theta_sd, mo.seed, mo.sequence);   // (uniform)
    else if (TRIG) { c = cs[2 * (size_t)p]; sn = cs[2 * (size_t)p + 1]; }
    if (lane == 0) {
        s_pose[0] = x; s_pose[1] = y; s_pose[2] = th;
        if (TRIG) { s_pose[3] = c; s_pose[4] = sn; }
        if (mo.on) {
            pose[3 * (size_t)p] = x; pose[3 * (size_t)p + 1] = y; pose[3 * (size_t)p + 2] = th;
            cs[2 * (size_t)p] = c; cs[2 * (size_t)p + 1] = sn;
        }
    }
    return th;
}
