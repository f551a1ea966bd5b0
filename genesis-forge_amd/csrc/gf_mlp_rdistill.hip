// gf_mlp_rdistill.hip — gf_mlp_recurrent_distill_act (include/gf_step.h has the contract): the collection step of distillation with a
// recurrent student.  Every device function is gf_mlp.hip's, compiled here with GF_BODIES_ONLY: the walk of gf_mlp_recurrent_act
// (rnn_forward: normaliser, cell, MLP) on the grid of gf_mlp_distill_act, with its finish (mlp_distill_finish).
// A translation unit of its own because the kernel's mere presence in gf_mlp.hip's changed the code the compiler emitted for
// mlp_recurrent_act_kernel — same source, same 193 VGPRs, another scalar allocation, 28 instructions more — and the recurrent PPO
// collection step measured 0.5 % slower for it (profiles/r27_recurrent_distill.md); built apart, that kernel's instruction stream is
// the one it had.
#define GF_BODIES_ONLY
#include "gf_mlp.hip"
#undef GF_BODIES_ONLY

namespace gf {

// gf_mlp_recurrent_distill_act: gf_mlp_distill_act's grid (y = 0 the student, y = 1 the teacher) over gf_mlp_recurrent_act's walk — the
// two LDS buffers, one workgroup per CU — and the distill finish.  One instance, as mlp_recurrent_act_kernel.
__global__ __launch_bounds__(kMlpBlock, 1) void mlp_recurrent_distill_kernel(const GfMlpRecurrentDistillArgs ra, const int vec_rows) {
    __shared__ RnnSmem sm;
    const GfMlpDistillArgs& a = ra.act;
    const bool is_teacher = blockIdx.y == 1;
    const GfMlpNet& net = is_teacher ? a.teacher : a.student;
    const GfRnnCell& cell = is_teacher ? ra.teacher_cell : ra.student_cell;
    const int64_t row0 = (int64_t)blockIdx.x * kMlpRows;

    const int A = rnn_forward(sm, net, cell, row0, a.num_envs);
    mlp_distill_finish(a, sm.m, is_teacher, A, row0, vec_rows);
}

}  // namespace gf

extern "C" __attribute__((visibility("default"))) int gf_mlp_recurrent_distill_act(const GfMlpRecurrentDistillArgs* ra, void* stream) {
    if (!ra) return GF_E_NULL;
    const GfMlpDistillArgs* a = &ra->act;
    int A = 0;
    int rc = gf::mlp_distill_check(*a, &A);
    if (rc != GF_OK) return rc;
    rc = gf::rnn_check_cell(ra->student_cell, true);
    if (rc != GF_OK) return rc;
    rc = gf::rnn_check_cell(ra->teacher_cell, true);
    if (rc != GF_OK) return rc;
    if (ra->student_cell.type == GF_RNN_NONE && ra->teacher_cell.type == GF_RNN_NONE) return GF_E_UNSUPPORTED;   // gf_mlp_distill_act's launch
    if (a->num_envs == 0) return GF_OK;
    const int64_t tiles = gf::mlp_tiles(a->num_envs);
    if (tiles < 0) return GF_E_RANGE;
    const int vec_rows = gf::mlp_vec_rows({a->noise, a->actions, a->actions_out, a->std}, A);
    gf::klaunch(gf::mlp_recurrent_distill_kernel, dim3((unsigned)tiles, 2u), dim3(gf::kMlpBlock), 0, (hipStream_t)stream, *ra, vec_rows);
    return gf::launch_status();
}
