// gf_distill.hip — gf_bc_loss: the behaviour-cloning loss of one time step of a distillation update (rsl_rl's Distillation.update:
// loss_fn(student mean, stored teacher actions), mse or huber) and its gradient w.r.t. the student's mean.  include/gf_step.h has the
// contract; not a phase of the step.
//
// The shape of gf_mirror_loss: one lane per row walks its A columns; the workgroup's sum of the per-element losses (double: wave
// butterfly, then the four waves in order) is one record of the workspace, a one-workgroup launch sums the records in a fixed order.
// The gradient needs no sum: it is written by the lane that computed d.  R 8A, W 4A bytes per row.
#include "gf_launch.h"
#include "gf_reduce.h"

namespace gf {

constexpr int kBcBlock = GF_BC_LOSS_BLOCK_ROWS;
constexpr int kBcFinBlock = 256;

static_assert(kBcBlock == kSumBlock, "block_wave_sums folds four waves");

template <int TYPE>
__global__ __launch_bounds__(kBcBlock) void bc_loss_rows_kernel(const GfBcLossArgs a) {
    __shared__ double s_w[kBcBlock / GF_WAVE];
    const int64_t N = a.num_rows;
    const int64_t i = (int64_t)blockIdx.x * kBcBlock + threadIdx.x;
    const int A = a.num_actions;
    double acc = 0.0;
    if (i < N) {
        const GF_GLOBAL float* mu = G(a.mu) + i * A;
        const GF_GLOBAL float* tg = G(a.target) + i * A;
        GF_GLOBAL float* g = a.grad ? G(a.grad) + i * A : nullptr;
        const float inv = 1.0f / (float)(N * A);   // mean's backward: grad / numel
        for (int j = 0; j < A; ++j) {
            const float d = mu[j] - tg[j];
            if (TYPE == GF_BC_LOSS_MSE) {
                acc += (double)d * (double)d;
                if (g) g[j] = inv * (2.0f * d);   // pow(2)'s backward: 2·d
            } else {   // torch's huber_loss, delta 1: the two branches meet at |d| == 1, where the quadratic one's gradient is taken
                const double ad = fabs((double)d);
                acc += ad < 1.0 ? 0.5 * ad * ad : ad - 0.5;
                if (g) g[j] = inv * fminf(fmaxf(d, -1.0f), 1.0f);
            }
        }
    }
    block_wave_sums(acc, s_w);
    if (threadIdx.x == 0) G(reinterpret_cast<double*>(a.workspace))[blockIdx.x] = fold_wave_sums(s_w);
}

__global__ __launch_bounds__(kBcFinBlock) void bc_loss_finalize_kernel(const GfBcLossArgs a, const int64_t nb) {
    finalize_mean_loss<kBcFinBlock>(a.workspace, nb, a.num_rows, a.num_actions, a.out, a.sums);   // sums: mean_behavior_loss
}

}  // namespace gf

extern "C" __attribute__((visibility("default"))) int gf_bc_loss(const GfBcLossArgs* a, void* stream) {
    if (!a || !a->mu || !a->target || !a->out || !a->workspace) return GF_E_NULL;
    if (a->num_rows < 0 || a->num_actions < 1 || (a->loss_type != GF_BC_LOSS_MSE && a->loss_type != GF_BC_LOSS_HUBER)) return GF_E_RANGE;
    if (a->num_rows == 0) return GF_OK;
    const int64_t nb = (a->num_rows + gf::kBcBlock - 1) / gf::kBcBlock;
    if (nb > 0x7fffffff) return GF_E_RANGE;
    if (a->workspace_bytes < GF_BC_LOSS_WORKSPACE_BYTES(a->num_rows) || (reinterpret_cast<uintptr_t>(a->workspace) & 7u)) return GF_E_RANGE;
    hipStream_t s = (hipStream_t)stream;
    if (a->loss_type == GF_BC_LOSS_MSE) gf::klaunch(gf::bc_loss_rows_kernel<GF_BC_LOSS_MSE>, dim3((unsigned)nb), dim3(gf::kBcBlock), 0, s, *a);
    else gf::klaunch(gf::bc_loss_rows_kernel<GF_BC_LOSS_HUBER>, dim3((unsigned)nb), dim3(gf::kBcBlock), 0, s, *a);
    gf::klaunch(gf::bc_loss_finalize_kernel, dim3(1), dim3(gf::kBcFinBlock), 0, s, *a, nb);
    return gf::launch_status();
}
