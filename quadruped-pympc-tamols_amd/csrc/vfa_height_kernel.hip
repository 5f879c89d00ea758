// vfa_height_kernel.hip -- the 'height' foothold strategy behind the apex gate, batched and device-resident
// (srbd_vfa_height_step_device / srbd_vfa_height_step_scenes_device, include/srbd_mpc.h).
//
// Restates VisualFootholdAdaptation.compute_adaptation, strategy 'height'
// (quadruped_pympc/helpers/visual_foothold_adaptation.py:145-151: each reference foothold's z becomes the heightmap's
// nearest-point height + 0.02), inside the gate of quadruped_pympc/interfaces/wb_interface.py:230-246.
// Grid (4 legs, E environments), rows * cols threads rounded up to whole waves.  Block (leg, e):
//   gate  : tamols_batch_body<GATED>'s -- wave 0 reads d_stc[e], contact[e] and the block's own word
//           d_vfa[e].initialized[leg], once, forms the mode (srbd_vfa.h vfa_mode) and hands it to the other waves
//           through one LDS word; a HOLD or PASS block copies its leg's ten slots and leaves, having read neither its
//           yaw, its scene index nor the scene;
//   rays  : a SEARCH block casts the leg's rows x cols rays around its seed (terrain_ray.h terrain_ray_point, one
//           lane per ray: heightmaps_out holds the bytes srbd_terrain_patches_device writes for that centre);
//   argmin: the nearest point to the seed under numpy.argmin's order (srbd_vfa.h vfa_height_before: a total order, so
//           the butterfly over a wave's lanes and the fold over the block's waves find the serial scan's point; the
//           lowest index wins ties; no atomics);
//   commit: thread 0 forms the foothold (vfa_height_result) and stores it through vfa_commit_leg with a NaN box.
// float64 and -ffp-contract=off: every value is the host chain's (srbd_vfa_mode -> srbd_vfa_height_search ->
// srbd_vfa_commit) bit for bit.
#include "srbd_vfa.h"
#include "terrain_ray.h"
#include "yaw_sincos.h"

namespace srbd {

constexpr int VFA_HEIGHT_THREADS = PATCH_BATCH_MAX_RAYS;
constexpr int VFA_HEIGHT_WAVES = (VFA_HEIGHT_THREADS + 63) / 64;

// The body is a device function the kernel below wraps, inlined into it: written as the kernel template itself, the
// SCENES instantiation crashes the compiler's optimizer (ROCm 7.2; tamols_batch_body met the same).
template <bool SCENES>
__device__ __forceinline__ void vfa_height_body(const VfaHeightJob& j) {
    __shared__ int32_t gate_mode;
    __shared__ TerrainDev lt;
    __shared__ double cs[2];
    __shared__ double wd[VFA_HEIGHT_WAVES], wz[VFA_HEIGHT_WAVES];
    __shared__ int wi[VFA_HEIGHT_WAVES];
    const int leg = blockIdx.x, e = blockIdx.y, tid = threadIdx.x;
    const size_t el = (size_t)e * 4 + leg;
    // ---- the gate: initialized[leg] is read here, by wave 0, and written only behind the barrier
    if (tid < 64) {
        double ct[4];
        for (int l = 0; l < 4; ++l) ct[l] = (double)j.contact[4 * (size_t)e + l];
        const int32_t m = vfa_mode(j.vfa[e].initialized[leg], j.stc + e, ct, j.apex_interval);
        if (tid == 0) gate_mode = m;
    }
    __syncthreads();
    const int32_t mode = __builtin_amdgcn_readfirstlane(gate_mode);  // block-uniform; tells the compiler so
    if (leg == 0 && tid == 0 && j.mode) j.mode[e] = mode;
    const double* seed = j.seeds + 12 * (size_t)e + 3 * leg;
    if (mode != SRBD_VFA_SEARCH) {
        if (tid < 10) {
            const double v = vfa_commit_slot(j.vfa + e, leg, mode, tid, seed, nullptr, nullptr, 0, j.footholds + 3 * el,
                                             j.boxes + 6 * el, j.valid + el);
            if (tid < 3 && j.ref) j.ref[24 * (size_t)e + 12 + 3 * leg + tid] = v;
        }
        return;
    }

    // ---- what the block's rays share: the scene's record (SCENES) and the yaw's cos / sin
    if (SCENES && tid < SCENE_RECORD_WORDS) {
        scene_record_load(j.table, j.scene, j.num_scenes, e, tid, &lt);
    } else if (tid == SCENE_RECORD_WORDS) {  // the next lane of wave 0
        yaw_sincos(j.yaws[e], cs[0], cs[1]);
    }
    __syncthreads();

    // ---- one ray per lane, and its distance from the seed
    const int nc = j.rows * j.cols;
    const double sx = seed[0], sy = seed[1];
    double bd = INFINITY, bz = 0.0;  // a lane without a ray comes after every point: +inf, an index past the patch
    int bi = 0x7fffffff;
    if (tid < nc) {
        TerrainDev trec;
        const TerrainDev* scene_rec = &j.t;
        if constexpr (SCENES) {  // out of LDS into registers
            trec = lt;
            scene_rec = &trec;
        }
        double o[3];
        terrain_ray_point(*scene_rec, sx, sy, cs[0], cs[1], j.rows, j.cols, tid / j.cols, tid % j.cols, j.dist_x,
                          j.dist_y, j.ray_z, o);
        if (j.hm_out) {
            double* h = j.hm_out + 3 * (el * nc + tid);
            h[0] = o[0];
            h[1] = o[1];
            h[2] = o[2];
        }
        bd = vfa_height_d2(o[0], o[1], sx, sy);
        bz = o[2];
        bi = tid;
    }

    // ---- argmin: butterfly within the wave, then thread 0 over the waves
    for (int m = 32; m >= 1; m >>= 1) {
        const double od = __shfl_xor(bd, m, 64), oz = __shfl_xor(bz, m, 64);
        const int oi = __shfl_xor(bi, m, 64);
        if (vfa_height_before(od, oi, bd, bi)) {
            bd = od;
            bi = oi;
            bz = oz;
        }
    }
    if ((tid & 63) == 0) {
        wd[tid >> 6] = bd;
        wi[tid >> 6] = bi;
        wz[tid >> 6] = bz;
    }
    __syncthreads();
    if (tid != 0) return;
    const int nw = ((int)blockDim.x + 63) >> 6;
    for (int w = 1; w < nw; ++w)
        if (vfa_height_before(wd[w], wi[w], bd, bi)) {
            bd = wd[w];
            bi = wi[w];
            bz = wz[w];
        }

    // ---- the leg's foothold into the state; the outputs are the state's (an older box where the ray missed)
    double f[3], b[6];
    int32_t valid;
    vfa_height_result(sx, sy, bz, f, &valid);
    for (int k = 0; k < 6; ++k) b[k] = NAN;
    vfa_commit_leg(j.vfa + e, leg, SRBD_VFA_SEARCH, seed, f, b, valid, j.footholds + 3 * el, j.boxes + 6 * el,
                   j.valid + el);
    if (j.seed_heights) j.seed_heights[el] = f[2];
    if (j.ref)
        for (int k = 0; k < 3; ++k) j.ref[24 * (size_t)e + 12 + 3 * leg + k] = f[k];
}

template <bool SCENES>
__global__ void __launch_bounds__(VFA_HEIGHT_THREADS) vfa_height_kernel(const VfaHeightJob j) {
    vfa_height_body<SCENES>(j);
}

void launch_vfa_height(const VfaHeightJob& j, hipStream_t s) {
    const int threads = (j.rows * j.cols + 63) / 64 * 64;  // whole waves, at most VFA_HEIGHT_THREADS
    if (j.table)
        hipLaunchKernelGGL(vfa_height_kernel<true>, dim3(4, j.E), dim3(threads), 0, s, j);
    else
        hipLaunchKernelGGL(vfa_height_kernel<false>, dim3(4, j.E), dim3(threads), 0, s, j);
}

}  // namespace srbd
