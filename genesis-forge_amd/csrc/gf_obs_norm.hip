// gf_obs_norm.hip — gf_obs_norm_update: the running mean / var / std / count of up to two observation normalisers (rsl_rl
// EmpiricalNormalization.update) in two launches.  include/gf_step.h has the contract; not a phase of the step.
//
// Launch 1 (grid: partial workgroups x sets): a workgroup owns the tiles b, b + P, … of 256 rows.  Up to 256 columns the lanes cover
// floor(256 / W) rows of W columns at a time — consecutive lanes read consecutive floats of consecutive rows — so a lane keeps ONE
// column as it walks down its rows; above 256 columns a lane keeps columns lane, lane + 256, … (up to four) of one row at a time.
// Either way the accumulators stay in registers: Σ(x - s) and Σ(x - s)² in float64 around s = the first element the lane reads (a
// sample of the column: the sums stay of the order of the spread, whatever the column's offset), eight rows of loads in flight.
// The lanes of a column then meet in LDS and the workgroup leaves {rows, mean[W], M2[W]} (M2 = Σ(x - mean)²) in the workspace.
// Launch 2 (grid: 1 x sets, 1 024 lanes): floor(1 024 / W) lanes per column each sum a slice of the P records, the column's first
// lane adds the slices in order, applies the update in float64 and stores mean, var (rounded to f32 once each), std = sqrtf(var) and
// — lane 0 — count.  Records are merged around the first record's mean (the pairwise-merge formula with the divisions taken out of
// the loop): Σx = N·m0 + Σ n_b (m_b - m0), M2 = Σ M2_b + Σ n_b (m_b - m0)² - (Σ n_b (m_b - m0))² / N.
// Every sum has a fixed order and no workgroup waits for another: bitwise reproducible.  Algorithmic traffic: R 4·N·W bytes per set.
#include "gf_launch.h"

namespace gf {

constexpr int kOnBlock = 256;
constexpr int kOnTile = GF_OBS_NORM_TILE_ROWS;
constexpr int kOnUnroll = 8;       // rows of loads in flight per lane
constexpr int kOnFinBlock = 1024;
static_assert(GF_MLP_MAX_INPUT_WIDTH <= 4 * kOnBlock && GF_MLP_MAX_INPUT_WIDTH <= kOnFinBlock, "a lane keeps at most four columns; launch 2 has a lane per column");

// column c of the set's input: element n is p[n * stride]
struct OnColumn {
    const GF_GLOBAL float* p;
    int64_t stride;
};

__device__ __forceinline__ OnColumn on_column(const GfObsNormSet& set, int c) {
    const float* rows = set.inputs[0].rows;
    int stride = set.inputs[0].row_stride ? set.inputs[0].row_stride : set.inputs[0].width, at = 0, k = c;
#pragma unroll
    for (int s = 0; s < GF_MLP_MAX_INPUTS; ++s) {
        const int w = s < set.num_inputs ? set.inputs[s].width : 0;
        const bool hit = k >= 0 && k < w;
        rows = hit ? set.inputs[s].rows : rows;
        stride = hit ? (set.inputs[s].row_stride ? set.inputs[s].row_stride : w) : stride;
        at = hit ? k : at;
        k -= w;
    }
    return OnColumn{G(rows) + at, (int64_t)stride};
}

// Q = columns per lane: 1 (W <= 256: floor(256 / W) lanes per column) or 4 (W > 256: one lane per column group)
template <int Q>
__device__ __forceinline__ void on_partial(const GfObsNormSet& set, const int64_t N, const int W, double* s_rec) {
    const int lane = (int)threadIdx.x;
    const int R = Q == 1 ? kOnBlock / W : 1;         // rows the workgroup reads at a time
    const int sub = Q == 1 ? lane / W : 0;           // this lane's row among them
    const bool lane_live = sub < R;
    OnColumn col[Q];
    bool live[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const int c = Q == 1 ? lane - sub * W : lane + q * kOnBlock;
        live[q] = lane_live && c < W;
        col[q] = on_column(set, live[q] ? c : 0);    // (a lane without a column reads column 0 and stores nothing)
    }
    const int64_t tiles = (N + kOnTile - 1) / kOnTile;
    const int64_t first = (int64_t)blockIdx.x * kOnTile + sub;   // (a lane past the end of a ragged only tile has no rows at all)
    double s[Q], s1[Q], s2[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        s[q] = lane_live && first < N ? (double)col[q].p[first * col[q].stride] : 0.0;
        s1[q] = s2[q] = 0.0;
    }
    int64_t rows = 0;
    if (lane_live) {
        for (int64_t t = blockIdx.x; t < tiles; t += gridDim.x) {
            const int64_t r0 = t * kOnTile;
            const int64_t r1 = r0 + kOnTile < N ? r0 + kOnTile : N;
            for (int64_t n = r0 + sub; n < r1; n += (int64_t)R * kOnUnroll) {
                float v[Q][kOnUnroll];
                bool ok[kOnUnroll];
#pragma unroll
                for (int j = 0; j < kOnUnroll; ++j) {
                    const int64_t nj = n + (int64_t)j * R;
                    ok[j] = nj < r1;
#pragma unroll
                    for (int q = 0; q < Q; ++q) v[q][j] = col[q].p[(ok[j] ? nj : n) * col[q].stride];
                }
#pragma unroll
                for (int j = 0; j < kOnUnroll; ++j) {
                    rows += ok[j] ? 1 : 0;
#pragma unroll
                    for (int q = 0; q < Q; ++q) {
                        const double d = ok[j] ? (double)v[q][j] - s[q] : 0.0;
                        s1[q] += d;
                        s2[q] += d * d;
                    }
                }
            }
        }
    }
    // this lane's records: (rows, mean, M2)
    const double k = (double)rows;
    double mean[Q], m2[Q];
#pragma unroll
    for (int q = 0; q < Q; ++q) {
        const double t = rows ? s1[q] / k : 0.0;
        const double r = s2[q] - s1[q] * t;
        mean[q] = rows ? s[q] + t : 0.0;
        m2[q] = r > 0.0 ? r : 0.0;
    }
    GF_GLOBAL double* rec = G(reinterpret_cast<double*>(set.workspace)) + (int64_t)blockIdx.x * (1 + 2 * (int64_t)W);
    if (Q != 1) {   // the lane owns its columns
        if (lane == 0) rec[0] = k;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const int c = lane + q * kOnBlock;
            if (live[q]) {
                rec[1 + c] = mean[q];
                rec[1 + W + c] = m2[q];
            }
        }
        return;
    }
    // the R lanes of a column, merged in row order by the column's first lane around its own mean (it has the most rows)
    s_rec[lane * 3] = k;
    s_rec[lane * 3 + 1] = mean[0];
    s_rec[lane * 3 + 2] = m2[0];
    __syncthreads();
    if (lane >= W) return;
    const double m0 = mean[0];
    double tn = 0.0, a1 = 0.0, a2 = 0.0, am = 0.0;
    for (int r = 0; r < R; ++r) {
        const double* e = s_rec + (lane + r * W) * 3;
        const double kr = e[0], dm = e[1] - m0;   // (a lane without rows: kr = 0 adds nothing)
        tn += kr;
        a1 += kr * dm;
        a2 += kr * (dm * dm);
        am += e[2];
    }
    const double t = a1 / tn;   // (tn >= 1: every workgroup of the grid has a tile)
    const double between = a2 - a1 * t;
    if (lane == 0) rec[0] = tn;
    rec[1 + lane] = m0 + t;
    rec[1 + W + lane] = am + (between > 0.0 ? between : 0.0);
}

__device__ __forceinline__ int on_width(const GfObsNormSet& set) {
    int W = 0;
    for (int s = 0; s < set.num_inputs; ++s) W += set.inputs[s].width;
    return W;
}

__global__ __launch_bounds__(kOnBlock) void obs_norm_partial_kernel(const GfObsNormArgs a) {
    __shared__ double s_rec[kOnBlock * 3];
    const GfObsNormSet& set = a.sets[blockIdx.y];
    const int W = on_width(set);
    if (W <= kOnBlock) on_partial<1>(set, a.num_rows, W, s_rec);
    else on_partial<4>(set, a.num_rows, W, s_rec);
}

__global__ __launch_bounds__(kOnFinBlock) void obs_norm_finalize_kernel(const GfObsNormArgs a, const int num_partials) {
    __shared__ double s_sum[3][kOnFinBlock];
    const GfObsNormSet& set = a.sets[blockIdx.y];
    const int64_t count = *G(set.count);   // (this workgroup is the only one that reads or writes it)
    if (set.until >= 0 && count >= set.until) return;   // frozen: nothing of the set is written (workgroup-uniform)
    const int W = on_width(set);
    const int tid = (int)threadIdx.x;
    const int J = kOnFinBlock / W;         // lanes per column: lane (j, c) sums the records j, j + J, …
    const int j = tid / W, c = tid - j * W;
    const int64_t stride = 1 + 2 * (int64_t)W;
    const GF_GLOBAL double* ws = G(reinterpret_cast<const double*>(set.workspace));
    const double m0 = j < J ? ws[1 + c] : 0.0;   // the first record's mean (it has a full tile unless it is the only one)
    double a1 = 0.0, a2 = 0.0, am = 0.0;
    if (j < J) {
        for (int b = j; b < num_partials; b += J) {
            const GF_GLOBAL double* rec = ws + b * stride;
            const double nb = rec[0], dm = rec[1 + c] - m0;
            a1 += nb * dm;
            a2 += nb * (dm * dm);
            am += rec[1 + W + c];
        }
    }
    s_sum[0][tid] = a1;
    s_sum[1][tid] = a2;
    s_sum[2][tid] = am;
    __syncthreads();
    if (tid >= W) return;
    a1 = a2 = am = 0.0;
    for (int i = 0; i < J; ++i) {
        a1 += s_sum[0][tid + i * W];
        a2 += s_sum[1][tid + i * W];
        am += s_sum[2][tid + i * W];
    }
    const double n = (double)a.num_rows;
    const double t = a1 / n;
    const double between = a2 - a1 * t;
    const double mx = m0 + t;
    const double vx = (am + (between > 0.0 ? between : 0.0)) / n;
    // rsl_rl's update lines, in float64 from the f32 state
    const double mean = (double)G(set.mean)[tid], var = (double)G(set.var)[tid];
    const int64_t count1 = count + a.num_rows;
    const double rate = n / (double)count1;
    const double d = mx - mean;
    const double mean1 = mean + rate * d;
    const double var1 = var + rate * (vx - var + d * (mx - mean1));
    const float var_f = (float)var1;
    G(set.mean)[tid] = (float)mean1;
    G(set.var)[tid] = var_f;
    G(set.std)[tid] = sqrtf(var_f);
    if (tid == 0) *G(set.count) = count1;
}

}  // namespace gf

extern "C" __attribute__((visibility("default"))) int gf_obs_norm_update(const GfObsNormArgs* a, void* stream) {
    if (!a) return GF_E_NULL;
    if (a->num_rows < 0 || a->num_sets < 1 || a->num_sets > GF_OBS_NORM_MAX_SETS) return GF_E_RANGE;
    for (int i = 0; i < a->num_sets; ++i) {
        const GfObsNormSet& set = a->sets[i];
        if (set.num_inputs < 1 || set.num_inputs > GF_MLP_MAX_INPUTS) return GF_E_RANGE;
        int64_t W = 0;
        for (int s = 0; s < set.num_inputs; ++s) {
            if (!set.inputs[s].rows) return GF_E_NULL;
            if (set.inputs[s].width < 1 || (set.inputs[s].row_stride && set.inputs[s].row_stride < set.inputs[s].width)) return GF_E_RANGE;
            W += set.inputs[s].width;
        }
        if (W > GF_MLP_MAX_INPUT_WIDTH) return GF_E_RANGE;
        if (!set.mean || !set.var || !set.std || !set.count || !set.workspace) return GF_E_NULL;
        if (set.workspace_bytes < GF_OBS_NORM_WORKSPACE_BYTES(a->num_rows, W) || (reinterpret_cast<uintptr_t>(set.workspace) & 7u) ||
            (reinterpret_cast<uintptr_t>(set.count) & 7u))
            return GF_E_RANGE;
    }
    if (a->num_rows == 0) return GF_OK;
    const int partials = (int)GF_OBS_NORM_PARTIALS(a->num_rows);
    hipStream_t s = (hipStream_t)stream;
    gf::klaunch(gf::obs_norm_partial_kernel, dim3((unsigned)partials, (unsigned)a->num_sets), dim3(gf::kOnBlock), 0, s, *a);
    gf::klaunch(gf::obs_norm_finalize_kernel, dim3(1u, (unsigned)a->num_sets), dim3(gf::kOnFinBlock), 0, s, *a, partials);
    return gf::launch_status();
}
