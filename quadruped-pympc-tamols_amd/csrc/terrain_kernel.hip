// terrain_kernel.hip -- heightmap patches by vertical ray casts against a device-resident scene
// (C-ABI in include/srbd_mpc.h, srbd_terrain_*).
//
// Replaces gym_quadruped's HeightMap.update_height_map, which casts one MuJoCo ray per patch point
// on the CPU (quadruped_pympc/interfaces/wb_interface.py:233-234; HeightMap(13, 7, 0.04, 0.04) at
// simulation/simulation.py:490-511).  One lane per ray; every lane of a launch walks the same
// primitive list, so the primitive loads are wave-uniform (scalar-cache broadcasts).  float64 and
// -ffp-contract=off: the points are bit-identical to oracle/terrain_oracle.py.
#include <math.h>

#include <algorithm>
#include <string>
#include <vector>

#include "terrain_ray.h"
#include "yaw_sincos.h"

namespace srbd {

__global__ void __launch_bounds__(256) terrain_patch_kernel(const TerrainDev t, const PatchJob j) {
    const int per = j.rows * j.cols;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= j.npatch * per) return;
    const int p = g / per, r = g % per, i = r / j.cols, k = r % j.cols;
    terrain_ray_point(t, j.centers[3 * p], j.centers[3 * p + 1], j.cs_yaw[2 * p], j.cs_yaw[2 * p + 1], j.rows, j.cols,
                      i, k, j.dist_x, j.dist_y, j.ray_z, j.out + 3 * (size_t)g);
}

void launch_terrain_patches(const TerrainDev& t, const PatchJob& j, hipStream_t s) {
    const int n = j.npatch * j.rows * j.cols;
    hipLaunchKernelGGL(terrain_patch_kernel, dim3((n + 255) / 256), dim3(256), 0, s, t, j);
}

// ------------------------------------------------------------------ device-resident height scans
// srbd_terrain_patches_device / srbd_terrain_set_patches_device: grid (K patches, E environments), one lane per ray.
// Wave 0 prepares what the block's rays share -- the yaw's cos / sin (yaw_sincos.h, one lane: the bits
// srbd_tamols_batch_device's kernel forms) and, SCENES, the environment's scene: scene[e] read once, bounds-checked,
// the record's 8-byte words copied into LDS or the empty scene's formed there (terrain_ray.h scene_record_load) -- and
// every lane then casts terrain_ray_point's ray, so a point holds the bytes terrain_patch_kernel and the TAMOLS
// launches write for the same centre, yaw and lattice.  Every ray walks the whole scene: the primitive loads are block-uniform.
static_assert(PATCH_BATCH_MAX_RAYS == TAMOLS_MAXCAND, "one lattice limit for the scans and the searches");

template <bool SCENES>
__global__ void __launch_bounds__(PATCH_BATCH_MAX_RAYS) terrain_patch_batch_kernel(const PatchBatchJob j) {
    __shared__ TerrainDev lt;
    __shared__ double cs[2];
    const int k = blockIdx.x, e = blockIdx.y, tid = threadIdx.x;
    if (SCENES && tid < SCENE_RECORD_WORDS) {
        scene_record_load(j.table, j.scene, j.num_scenes, e, tid, &lt);
    } else if (tid == SCENE_RECORD_WORDS) {  // the next lane of wave 0
        yaw_sincos(j.yaws[e], cs[0], cs[1]);
    }
    __syncthreads();
    const int nc = j.rows * j.cols;
    if (tid >= nc) return;
    TerrainDev trec;
    const TerrainDev* scene_rec = &j.t;
    if constexpr (SCENES) {  // out of LDS into registers
        trec = lt;
        scene_rec = &trec;
    }
    const double* c = j.centers + 3 * ((size_t)e * j.K + k);
    const size_t at = ((size_t)e * j.K + k) * nc + tid;
    if (j.points && !j.heights) {  // straight to the caller's array, as terrain_patch_kernel
        terrain_ray_point(*scene_rec, c[0], c[1], cs[0], cs[1], j.rows, j.cols, tid / j.cols, tid % j.cols, j.dist_x,
                          j.dist_y, j.ray_z, j.points + 3 * at);
        return;
    }
    double o[3];
    terrain_ray_point(*scene_rec, c[0], c[1], cs[0], cs[1], j.rows, j.cols, tid / j.cols, tid % j.cols, j.dist_x,
                      j.dist_y, j.ray_z, o);
    if (j.points) {
        double* p = j.points + 3 * at;
        p[0] = o[0];
        p[1] = o[1];
        p[2] = o[2];
    }
    j.heights[at] = o[2];  // consecutive lanes, consecutive doubles
}

void launch_patch_batch(const PatchBatchJob& j, hipStream_t s) {
    const int threads = (j.rows * j.cols + 63) / 64 * 64;  // whole waves, at most PATCH_BATCH_MAX_RAYS
    if (j.table)
        hipLaunchKernelGGL(terrain_patch_batch_kernel<true>, dim3(j.K, j.E), dim3(threads), 0, s, j);
    else
        hipLaunchKernelGGL(terrain_patch_batch_kernel<false>, dim3(j.K, j.E), dim3(threads), 0, s, j);
}

}  // namespace srbd

using namespace srbd;

static std::string g_terrain_error;

int srbd::terrain_fail(srbd_terrain* t, int code, const std::string& m) {
    (t ? t->err : g_terrain_error) = m;
    return code;
}

#define TER_TRY(t, expr)                                                                       \
    do {                                                                                       \
        hipError_t _e = (expr);                                                                \
        if (_e != hipSuccess) return terrain_fail((t), SRBD_E_HIP, std::string(#expr) + ": " + hipGetErrorString(_e)); \
    } while (0)

// What srbd_terrain_create refuses of a scene's arguments (NULL: nothing), before any HIP call; a scene of a set
// (srbd_terrain_set_create) is checked by the same function.
static const char* scene_refused(const srbd_terrain_prim* prims, int32_t nprims, const double* hfield, int32_t hf_nx,
                                 int32_t hf_ny, double hf_dx, double hf_dy) {
    if (nprims < 0 || (nprims > 0 && !prims)) return "bad arguments";
    if (hfield && (hf_nx < 2 || hf_ny < 2 || !(hf_dx > 0.0) || !(hf_dy > 0.0)))
        return "height field needs >= 2 x 2 points and positive spacing";
    for (int q = 0; q < nprims; ++q)
        if (prims[q].type != SRBD_PRIM_BOX && prims[q].type != SRBD_PRIM_CYLINDER) return "unknown primitive type";
    return nullptr;
}

// The device scene's box-yaw pairs: cs[2 q], cs[2 q + 1] = cos, sin of prims[q].yaw (the host's libm).  The one place
// they are formed, so a scene alone and the same scene in a set hold the same bits.
static void prim_yaw_cs(const srbd_terrain_prim* prims, int32_t nprims, double* cs) {
    for (int q = 0; q < nprims; ++q) {
        cs[2 * q] = cos(prims[q].yaw);
        cs[2 * q + 1] = sin(prims[q].yaw);
    }
}

extern "C" void srbd_terrain_destroy(srbd_terrain* t) {
    if (!t) return;
    (void)hipSetDevice(t->device);
    if (t->stream) (void)hipStreamSynchronize(t->stream);
    (void)hipFree(t->d_prims);
    (void)hipFree(t->d_cs);
    (void)hipFree(t->d_hf);
    (void)hipFree(t->d_job);
    (void)hipFree(t->d_out);
    if (t->h_job) (void)hipHostFree(t->h_job);
    if (t->stream) (void)hipStreamDestroy(t->stream);
    delete t;
}

extern "C" const char* srbd_terrain_last_error(const srbd_terrain* t) {
    return t ? t->err.c_str() : g_terrain_error.c_str();
}

extern "C" int srbd_terrain_create(int32_t device_id, const srbd_terrain_prim* prims, int32_t nprims, int32_t has_ground,
                                   double ground_z, const double* hfield, int32_t hf_nx, int32_t hf_ny, double hf_x0,
                                   double hf_y0, double hf_dx, double hf_dy, double miss_z, srbd_terrain** out) {
    if (!out) return terrain_fail(nullptr, SRBD_E_INVALID, "bad arguments");
    if (const char* why = scene_refused(prims, nprims, hfield, hf_nx, hf_ny, hf_dx, hf_dy))
        return terrain_fail(nullptr, SRBD_E_INVALID, why);
    *out = nullptr;
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0 || device_id < 0 || device_id >= ndev)
        return terrain_fail(nullptr, SRBD_E_NODEVICE, "no HIP device visible (this library has no CPU fallback)");
    srbd_terrain* t = new srbd_terrain();
    t->device = device_id;
    t->dev.nprims = nprims;
    t->dev.has_ground = has_ground != 0;
    t->dev.ground_z = ground_z;
    t->dev.miss_z = miss_z;
    t->dev.hf_nx = hfield ? hf_nx : 0;
    t->dev.hf_ny = hfield ? hf_ny : 0;
    t->dev.hf_x0 = hf_x0;
    t->dev.hf_y0 = hf_y0;
    t->dev.hf_dx = hf_dx;
    t->dev.hf_dy = hf_dy;
    {
        const auto ok = [](double v) { return std::isfinite(v) && fabs(v) < 1e30; };
        bool b = !has_ground || ok(ground_z);  // miss_z: checked per call (a ray below the ground misses)
        for (int q = 0; b && q < nprims; ++q) {
            const srbd_terrain_prim& p = prims[q];
            b = ok(p.cx) && ok(p.cy) && ok(p.cz) && ok(p.a) && ok(p.b) && ok(p.c) && ok(p.yaw);
        }
        if (hfield) {
            b = b && ok(hf_x0) && ok(hf_y0) && ok(hf_dx) && ok(hf_dy);
            for (size_t i = 0; b && i < (size_t)hf_nx * hf_ny; ++i) b = ok(hfield[i]);
        }
        t->bounded = b;
    }
    auto bad = [&](hipError_t e) {
        const std::string m = std::string("terrain upload: ") + hipGetErrorString(e);
        srbd_terrain_destroy(t);
        return terrain_fail(nullptr, SRBD_E_HIP, m);
    };
    hipError_t e;
    if ((e = hipSetDevice(device_id)) != hipSuccess) return bad(e);
    if ((e = hipStreamCreateWithFlags(&t->stream, hipStreamNonBlocking)) != hipSuccess) return bad(e);
    if (nprims > 0) {
        std::vector<double> cs(2 * (size_t)nprims);
        prim_yaw_cs(prims, nprims, cs.data());
        if ((e = hipMalloc((void**)&t->d_prims, sizeof(srbd_terrain_prim) * nprims)) != hipSuccess) return bad(e);
        if ((e = hipMalloc((void**)&t->d_cs, sizeof(double) * 2 * nprims)) != hipSuccess) return bad(e);
        if ((e = hipMemcpy(t->d_prims, prims, sizeof(srbd_terrain_prim) * nprims, hipMemcpyHostToDevice)) != hipSuccess)
            return bad(e);
        if ((e = hipMemcpy(t->d_cs, cs.data(), sizeof(double) * 2 * nprims, hipMemcpyHostToDevice)) != hipSuccess)
            return bad(e);
    }
    if (hfield) {
        const size_t b = sizeof(double) * (size_t)hf_nx * hf_ny;
        if ((e = hipMalloc((void**)&t->d_hf, b)) != hipSuccess) return bad(e);
        if ((e = hipMemcpy(t->d_hf, hfield, b, hipMemcpyHostToDevice)) != hipSuccess) return bad(e);
    }
    t->dev.prims = t->d_prims;
    t->dev.cs = t->d_cs;
    t->dev.hf = t->d_hf;
    *out = t;
    return SRBD_OK;
}

// ------------------------------------------------------------------ a set of scenes (srbd_terrain_set_*)
static thread_local std::string g_terrain_set_error;

int srbd::terrain_set_fail(srbd_terrain_set* set, int code, const std::string& m) {
    (set ? set->err : g_terrain_set_error) = m;
    return code;
}

extern "C" void srbd_terrain_set_destroy(srbd_terrain_set* set) {
    if (!set) return;
    (void)hipSetDevice(set->device);
    (void)hipFree(set->d_prims);
    (void)hipFree(set->d_cs);
    (void)hipFree(set->d_hf);
    (void)hipFree(set->d_table);
    delete set;
}

extern "C" const char* srbd_terrain_set_last_error(const srbd_terrain_set* set) {
    return set ? set->err.c_str() : g_terrain_set_error.c_str();
}

extern "C" int srbd_terrain_set_num_scenes(const srbd_terrain_set* set) {
    return set ? set->num_scenes : SRBD_E_INVALID;
}

extern "C" int srbd_terrain_set_create(int32_t device_id, const srbd_terrain_scene* scenes, int32_t num_scenes,
                                       srbd_terrain_set** out) {
    constexpr int MAX_SCENES = 4096;
    if (!out) return terrain_set_fail(nullptr, SRBD_E_INVALID, "srbd_terrain_set_create: null out");
    *out = nullptr;
    if (!scenes) return terrain_set_fail(nullptr, SRBD_E_INVALID, "srbd_terrain_set_create: null scenes");
    if (num_scenes < 1 || num_scenes > MAX_SCENES)
        return terrain_set_fail(nullptr, SRBD_E_INVALID, "srbd_terrain_set_create: num_scenes must be 1..4096");
    // every scene as srbd_terrain_create checks it; the concatenated arrays are indexed with int
    int64_t np_all = 0, nh_all = 0;
    for (int s = 0; s < num_scenes; ++s) {
        const srbd_terrain_scene& c = scenes[s];
        if (const char* why = scene_refused(c.prims, c.nprims, c.hfield, c.hf_nx, c.hf_ny, c.hf_dx, c.hf_dy))
            return terrain_set_fail(nullptr, SRBD_E_INVALID,
                                    "srbd_terrain_set_create: scene " + std::to_string(s) + ": " + why);
        np_all += c.nprims;
        if (c.hfield) nh_all += (int64_t)c.hf_nx * c.hf_ny;
        if (np_all > INT32_MAX || nh_all > INT32_MAX)
            return terrain_set_fail(nullptr, SRBD_E_INVALID,
                                    "srbd_terrain_set_create: scene " + std::to_string(s) +
                                        ": the scenes' primitives or height-field points together exceed 2^31 - 1");
    }
    int ndev = 0;
    if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0 || device_id < 0 || device_id >= ndev)
        return terrain_set_fail(nullptr, SRBD_E_NODEVICE,
                                "srbd_terrain_set_create: no HIP device visible (this library has no CPU fallback)");
    srbd_terrain_set* t = new srbd_terrain_set();
    t->device = device_id;
    t->num_scenes = num_scenes;
    auto bad = [&](hipError_t e) {
        const std::string m = std::string("srbd_terrain_set_create: upload: ") + hipGetErrorString(e);
        srbd_terrain_set_destroy(t);
        return terrain_set_fail(nullptr, e == hipErrorOutOfMemory ? SRBD_E_NOMEM : SRBD_E_HIP, m);
    };
    hipError_t e;
    if ((e = hipSetDevice(device_id)) != hipSuccess) return bad(e);
    if (np_all > 0) {
        if ((e = hipMalloc((void**)&t->d_prims, sizeof(srbd_terrain_prim) * (size_t)np_all)) != hipSuccess) return bad(e);
        if ((e = hipMalloc((void**)&t->d_cs, sizeof(double) * 2 * (size_t)np_all)) != hipSuccess) return bad(e);
    }
    if (nh_all > 0 && (e = hipMalloc((void**)&t->d_hf, sizeof(double) * (size_t)nh_all)) != hipSuccess) return bad(e);
    if ((e = hipMalloc((void**)&t->d_table, sizeof(TerrainDev) * (size_t)num_scenes)) != hipSuccess) return bad(e);
    // host images of the three arrays, scene after scene, and each scene's record pointing at its own slice
    std::vector<srbd_terrain_prim> prims((size_t)np_all);
    std::vector<double> cs(2 * (size_t)np_all), hf((size_t)nh_all);
    std::vector<TerrainDev> table((size_t)num_scenes);
    size_t po = 0, ho = 0;  // the scene's first primitive and first height-field point
    for (int s = 0; s < num_scenes; ++s) {
        const srbd_terrain_scene& c = scenes[s];
        TerrainDev& d = table[s];
        d = TerrainDev{};
        d.nprims = c.nprims;
        d.has_ground = c.has_ground != 0;
        d.ground_z = c.ground_z;
        d.miss_z = c.miss_z;
        d.hf_nx = c.hfield ? c.hf_nx : 0;
        d.hf_ny = c.hfield ? c.hf_ny : 0;
        d.hf_x0 = c.hf_x0;
        d.hf_y0 = c.hf_y0;
        d.hf_dx = c.hf_dx;
        d.hf_dy = c.hf_dy;
        if (c.nprims > 0) {
            std::copy(c.prims, c.prims + c.nprims, prims.begin() + po);
            prim_yaw_cs(c.prims, c.nprims, cs.data() + 2 * po);
            d.prims = t->d_prims + po;
            d.cs = t->d_cs + 2 * po;
            po += (size_t)c.nprims;
        }
        if (c.hfield) {
            const size_t n = (size_t)c.hf_nx * c.hf_ny;
            std::copy(c.hfield, c.hfield + n, hf.begin() + ho);
            d.hf = t->d_hf + ho;
            ho += n;
        }
    }
    if (np_all > 0) {
        if ((e = hipMemcpy(t->d_prims, prims.data(), sizeof(srbd_terrain_prim) * prims.size(), hipMemcpyHostToDevice)) !=
            hipSuccess)
            return bad(e);
        if ((e = hipMemcpy(t->d_cs, cs.data(), sizeof(double) * cs.size(), hipMemcpyHostToDevice)) != hipSuccess)
            return bad(e);
    }
    if (nh_all > 0 &&
        (e = hipMemcpy(t->d_hf, hf.data(), sizeof(double) * hf.size(), hipMemcpyHostToDevice)) != hipSuccess)
        return bad(e);
    if ((e = hipMemcpy(t->d_table, table.data(), sizeof(TerrainDev) * table.size(), hipMemcpyHostToDevice)) !=
        hipSuccess)
        return bad(e);
    *out = t;
    return SRBD_OK;
}

// Job inputs (centres, yaw cos / sin) staged through pinned memory and one H2D copy into d_job; the
// output buffer grows on demand.  Returns the device output pointer in *d_out.
int srbd::terrain_enqueue(srbd_terrain* t, const double* centers, const double* yaws, int npatch, int rows, int cols,
                    double dist_x, double dist_y, double ray_z, hipStream_t s, double** d_out) {
    if (!t || !centers || !yaws || npatch < 1 || rows < 1 || cols < 1)
        return terrain_fail(t, SRBD_E_INVALID, "bad patch arguments");
    const size_t need_out = (size_t)npatch * rows * cols * 3, need_job = 5 * (size_t)npatch;
    if (t->cap_job < need_job) {
        TER_TRY(t, hipStreamSynchronize(s));
        (void)hipFree(t->d_job);
        if (t->h_job) (void)hipHostFree(t->h_job);
        t->d_job = t->h_job = nullptr;
        t->cap_job = 0;
        TER_TRY(t, hipMalloc((void**)&t->d_job, sizeof(double) * need_job));
        TER_TRY(t, hipHostMalloc((void**)&t->h_job, sizeof(double) * need_job, hipHostMallocDefault));
        t->cap_job = need_job;
    }
    if (t->cap_out < need_out) {
        (void)hipFree(t->d_out);
        t->d_out = nullptr;
        TER_TRY(t, hipMalloc((void**)&t->d_out, sizeof(double) * need_out));
        t->cap_out = need_out;
    }
    // the previous call's copy out of h_job has completed: every call ends with a stream synchronise
    for (int p = 0; p < npatch; ++p) {
        for (int q = 0; q < 3; ++q) t->h_job[3 * p + q] = centers[3 * p + q];
        t->h_job[3 * npatch + 2 * p] = cos(yaws[p]);
        t->h_job[3 * npatch + 2 * p + 1] = sin(yaws[p]);
    }
    TER_TRY(t, hipMemcpyAsync(t->d_job, t->h_job, sizeof(double) * need_job, hipMemcpyHostToDevice, s));
    PatchJob j;
    j.centers = t->d_job;
    j.cs_yaw = t->d_job + 3 * npatch;
    j.npatch = npatch;
    j.rows = rows;
    j.cols = cols;
    j.dist_x = dist_x;
    j.dist_y = dist_y;
    j.ray_z = ray_z;
    j.out = t->d_out;
    launch_terrain_patches(t->dev, j, s);
    TER_TRY(t, hipGetLastError());
    *d_out = t->d_out;
    return SRBD_OK;
}

extern "C" int srbd_terrain_patches(srbd_terrain* t, const double* centers, const double* yaws, int32_t npatch,
                                    int32_t rows, int32_t cols, double dist_x, double dist_y, double ray_z, double* out) {
    if (!t || !out) return terrain_fail(t, SRBD_E_INVALID, "bad arguments");
    TER_TRY(t, hipSetDevice(t->device));
    double* d_out = nullptr;
    if (int rc = terrain_enqueue(t, centers, yaws, npatch, rows, cols, dist_x, dist_y, ray_z, t->stream, &d_out))
        return rc;
    TER_TRY(t, hipMemcpyAsync(out, d_out, sizeof(double) * 3 * (size_t)npatch * rows * cols, hipMemcpyDeviceToHost,
                              t->stream));
    TER_TRY(t, hipStreamSynchronize(t->stream));
    return SRBD_OK;
}
