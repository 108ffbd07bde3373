// The fused training loss of csrc/ssim.hip -- (1 - lambda) L1 + lambda (1 - SSIM) in the marching-wave SSIM kernels' single pass, forward and
// backward -- and the plain mean-SSIM form, compiled for the HOST through the SIMT-on-CPU shim (raw buffer loads / stores with the hardware's
// out-of-range behaviour) and run through their own launchers (tests/test_simt_loss_cpu.py).  TEST INFRASTRUCTURE, never part of libgsr_hip.so.
#define __HIPCC__ 1
#include "hip/hip_runtime.h"
#include "ssim.hip"
#include "simt_runtime.h"
#include <vector>

static char g_err[256];
static int finish(const char* what) {
    if (!simt::launch_error) return 0;
    snprintf(g_err, sizeof(g_err), "%s: %s", what, simt::launch_error);
    simt::launch_error = nullptr;
    return -1;
}

extern "C" {

const char* simt_loss_last_error(void) { return g_err; }

// loss = (1 - lambda) mean|img1 - img2| + lambda (1 - SSIM(img1, img2)); dL_dimg1 for dL/dloss = upstream
int simt_train_loss(int planes, int H, int W, const float* img1, const float* img2, float lambda, float upstream, float* loss_out, float* dL_dimg1) {
    const size_t n = (size_t)planes * H * W;
    std::vector<float> partials(2 * (size_t)gsr_ssim_partial_count_impl(planes, H, W) + 64), a(n + 16), b(n + 16), c(n + 16);      // (SSIM and L1 parts)
    gsr_launch_train_loss_forward(planes, H, W, img1, img2, lambda, partials.data(), loss_out, a.data(), b.data(), c.data(), nullptr);
    if (finish("train loss forward")) return -1;
    gsr_launch_train_loss_backward(planes, H, W, img1, img2, &upstream, lambda, a.data(), b.data(), c.data(), dL_dimg1, nullptr);
    return finish("train loss backward");
}

// mean SSIM and its gradient (fused_ssim)
int simt_ssim_mean(int planes, int H, int W, const float* img1, const float* img2, float upstream, float* mean_out, float* dL_dimg1) {
    const size_t n = (size_t)planes * H * W;
    std::vector<float> partials((size_t)gsr_ssim_partial_count_impl(planes, H, W) + 64), a(n + 16), b(n + 16), c(n + 16);
    gsr_launch_ssim_mean_forward(planes, H, W, img1, img2, partials.data(), mean_out, a.data(), b.data(), c.data(), nullptr);
    if (finish("ssim mean forward")) return -1;
    gsr_launch_ssim_mean_backward(planes, H, W, img1, img2, &upstream, a.data(), b.data(), c.data(), dL_dimg1, nullptr);
    return finish("ssim mean backward");
}

// ---- launch plan and variant: the two wave targets on their own (the product option writes one value into both and clamps it at 256: here a few
// hundred rows have to reach the plans of a 1080p / 4K frame), the variant, and the plan a launch will take ----
void simt_loss_set_target_waves(int fwd, int bwd) { g_ssim_target_waves[0] = fwd; g_ssim_target_waves[1] = bwd; }
void simt_loss_set_variant(int v) { g_ssim_variant = v; }
// the product's own reset (gsr_set_option("ssim_target_waves", 0)) and the variant default
void simt_loss_restore_defaults(void) { gsr_set_ssim_target_waves(0); gsr_set_ssim_variant(0); }
void simt_loss_get_target_waves(int* out2) { out2[0] = g_ssim_target_waves[0]; out2[1] = g_ssim_target_waves[1]; }
void simt_loss_march_plan(int planes, int H, int W, int bwd, int* out4 /*nsx, nsy, seg, lds*/) {
    const MarchPlan p = march_plan(planes, H, W, bwd);
    out4[0] = p.nsx; out4[1] = p.nsy; out4[2] = p.seg; out4[3] = (int)p.lds;
}

// the map-returning pair (FusedSSIMMap): SSIM map, and dL/dimg1 for a per-pixel dL/dmap
int simt_ssim_map(int planes, int H, int W, const float* img1, const float* img2, const float* dL_dmap, float* map_out, float* dL_dimg1) {
    const size_t n = (size_t)planes * H * W;
    std::vector<float> a(n + 16), b(n + 16), c(n + 16);
    gsr_launch_ssim_forward(planes, H, W, img1, img2, map_out, a.data(), b.data(), c.data(), nullptr);
    if (finish("ssim map forward")) return -1;
    gsr_launch_ssim_backward(planes, H, W, img1, img2, dL_dmap, a.data(), b.data(), c.data(), dL_dimg1, nullptr);
    return finish("ssim map backward");
}

// mean SSIM without derivative maps (the torch.no_grad() evaluation: always the LDS-tiled forward)
int simt_ssim_mean_no_maps(int planes, int H, int W, const float* img1, const float* img2, float* mean_out) {
    std::vector<float> partials((size_t)gsr_ssim_partial_count_impl(planes, H, W) + 64);
    gsr_launch_ssim_mean_forward(planes, H, W, img1, img2, partials.data(), mean_out, nullptr, nullptr, nullptr, nullptr);
    return finish("ssim mean forward without maps");
}

}  // extern "C"
