/*
 * gf_step.h — C ABI of the MI355X-native ManagedEnvironment manager-step pipeline.
 *
 * One entry point per phase of the reference's ManagedEnvironment.step()
 * (/root/reference/genesis_forge/managed_env.py:274-334).  Every function takes a POD
 * descriptor of caller-owned device buffers (row-major, contiguous, f32 unless noted)
 * plus the HIP stream to launch on, and returns an int status:
 *      0            success
 *      < 0          argument validation failure (GF_E_*)
 *      > 0          hipError_t of the failing runtime call
 * The phase entry points allocate nothing, never synchronise the device and keep no state between
 * calls: everything a launch reads or writes is named by its descriptor, so they are re-entrant per
 * (device, stream) and ownership never crosses the ABI.  What IS process-global, and
 * therefore not re-entrant, is diagnostic: the tuning switches of gf_set_option() (read once per
 * launch), the single-phase event profiler gf_profile_begin() / gf_profile_end() and the append-only
 * table of run-time programs (gf_post_program_register, thread-safe).  The opaque handles of
 * gf_run_ops_graph() / gf_event_create() belong to the caller that created them.
 * No torch types appear here; the Python host (genesis_forge_amd) hands over `tensor.data_ptr()`
 * values via ctypes.
 *
 * Conventions
 *   N = num_envs, D = controlled DOFs, L = tracked links of one ContactManager,
 *   C = contact slots, T/K = number of reward/termination terms, O = observation width.
 *   Masks are 1 byte per env (torch.bool).  Counters are int32.  Quaternions are (w,x,y,z).
 *   "draws": wherever the reference consumes torch's global RNG (Tensor.uniform_), the kernel
 *   takes either a dense array of U[0,1) floats (parity mode) or NULL, in which case it
 *   generates the same kind of draw with Philox4x32-10 keyed by (seed, stream, env, lane).
 */
#ifndef GF_STEP_H
#define GF_STEP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GF_ABI_VERSION 11

#define GF_MAX_TERMS 24          /* reward terms per manager          */
#define GF_MAX_TERM_TERMS 16     /* termination terms per manager     */
#define GF_MAX_OBS_ITEMS 24      /* observation items per manager     */
#define GF_MAX_CONTACT_VIEWS 4   /* ContactManagers visible to a term */
#define GF_MAX_COMMAND_VIEWS 4   /* CommandManagers visible to a term */
#define GF_MAX_EXT 16            /* opaque Python-evaluated columns   */
#define GF_MAX_LINK_IDS 32       /* target / with link ids            */
#define GF_MAX_RANGES 8          /* command ranges per CommandManager */
#define GF_MAX_OBS_WIDTH 256     /* single-frame observation width    */
#define GF_MAX_GAITS 4           /* gaits a GaitCommandManager samples from */

/* error codes */
#define GF_OK 0
#define GF_E_NULL (-1)      /* required pointer is NULL              */
#define GF_E_RANGE (-2)     /* size / count out of supported range   */
#define GF_E_OPCODE (-3)    /* unknown opcode in a term table        */
#define GF_E_SLOT (-4)      /* term references an unbound view/slot  */
#define GF_E_UNSUPPORTED (-5)

/* ------------------------------------------------------------------------------------------
 * Shared views
 * ---------------------------------------------------------------------------------------- */

/* World-frame base-link state of one entity, as returned by RigidEntity.get_pos/quat/vel/ang
 * (call sites: genesis_forge/utils.py:13-55, managers/entity_manager.py:130-146,189-195). */
typedef struct GfEntityView {
    const float* pos;      /* [N,3] */
    const float* quat;     /* [N,4] (w,x,y,z) */
    const float* lin_vel;  /* [N,3] world frame */
    const float* ang_vel;  /* [N,3] world frame */
} GfEntityView;

/* Buffers a ContactManager publishes (managers/contact/contact_manager.py:142-156,300-314). */
typedef struct GfContactView {
    const float* contacts;              /* [N,L,3] link-local net force  */
    const float* last_air_time;         /* [N,L] or NULL                 */
    const float* current_contact_time;  /* [N,L] or NULL                 */
    const float* link_vel;              /* [N,L,3] world link velocity (feet_slide, gait rewards) or NULL */
    const float* link_pos;              /* [N,L,3] world link position (foot_height_reward) or NULL */
    int32_t num_links;                  /* L */
    int32_t _pad;
} GfContactView;

/* CommandManager._command (managers/command/command_manager.py:77-81). */
typedef struct GfCommandView {
    const float* command;  /* [N,width], row n at command + n*stride */
    int32_t width;
    int32_t stride;        /* floats between rows; 0 = width (dense).  The gait manager's 14 observed columns live in 16-float rows */
} GfCommandView;

/* TerrainManager's map of the terrain (managers/terrain_manager.py:281-359): the height field after `* vertical_scale` and
 * the transpose of :354-359, i.e. rows index y and cols index x, plus the bounds get_terrain_height normalises with
 * (:117-136).  A NULL height_field is the "no height field" case of :112-114: every query returns origin_z. */
typedef struct GfTerrainView {
    const float* height_field;  /* [rows, cols] f32 metres, or NULL */
    int32_t rows;               /* H (y direction) */
    int32_t cols;               /* W (x direction) */
    float x_min;                /* (float)bounds[0] */
    float x_span;               /* (float)(bounds[1] - bounds[0]), the double difference rounded once (`div_(x_max - x_min)`) */
    float y_min;
    float y_span;
    float origin_z;
    int32_t _pad;
} GfTerrainView;

/* One row of a term table.  Meaning of p[]/i[] is per opcode (see enums below). */
typedef struct GfTerm {
    int32_t op;
    int32_t flags;
    float w;        /* rewards: (float)(weight*dt)  (reward_manager.py:185-186)  */
    float p[4];
    int32_t i[4];
    int32_t row;    /* rewards: row of episode_sums / term_out this term owns      */
} GfTerm;           /* 48 bytes */

/* Per-step scalar statistics, accumulated on device, read back lazily by the host.
 * These are the only cross-env reductions of the path; at world_size>1 the
 * summed block (cast to f64) is the payload of the single RCCL all-reduce.
 * Every `stats` pointer of this ABI addresses an array of GF_STATS_SHARDS blocks: workgroup b
 * accumulates into shard b % GF_STATS_SHARDS (1 024 waves adding to ONE word serialise at ≈ 88
 * atomics/µs; sharding removes that), and the reader sums the shards (flags: bitwise OR). */
#define GF_STATS_SHARDS 64
typedef struct GfStepStats {
    int32_t term_fired[GF_MAX_TERM_TERMS]; /* #envs for which termination term k fired (termination_manager.py:178-182) */
    int32_t reset_count;                   /* #envs reset this step (managed_env.py:308-323) */
    int32_t action_flags;                  /* bit0: NaN action seen, bit1: Inf action seen (position_action_manager.py:402-406) */
    int32_t contact_flags;                 /* bit0: non-finite contact force sanitised (contact_manager.py:399-403) */
    int32_t resample_count;                /* #envs whose command was resampled by command.step() */
    int32_t gait_count[GF_MAX_GAITS];      /* #envs currently on gait g, counted every step by gf_gait_step ("Metrics / gait_<name>_envs") */
    double reward_episode_sum[GF_MAX_TERMS]; /* Σ over reset envs of episode_sum[t]/episode_seconds (reward_manager.py:207-216) */
} GfStepStats;

/* ------------------------------------------------------------------------------------------
 * Phase A — GenesisEnv.step bookkeeping + PositionActionManager.step
 *   genesis_env.py:181-205; managers/action/base.py:67-82;
 *   managers/action/position_action_manager.py:376-419; position_within_limits.py:100-131
 * ---------------------------------------------------------------------------------------- */
enum { GF_ACTION_POSITION = 0, GF_ACTION_WITHIN_LIMITS = 1 };

typedef struct GfActionArgs {
    int32_t num_envs;
    int32_t num_dofs;
    int32_t mode;            /* GF_ACTION_* */
    int32_t check_finite;    /* !quiet_action_errors: set stats->action_flags bits */
    const float* actions_in; /* [N,D] policy output (never written) */
    const float* scale;      /* [D] */
    const float* offset;     /* [D] */
    const float* clip_lo;    /* [D] */
    const float* clip_hi;    /* [D] */
    float* env_actions;      /* [N,D] GenesisEnv._actions      (may be NULL: bookkeeping skipped) */
    float* env_last_actions; /* [N,D] GenesisEnv._last_actions */
    int32_t* episode_length; /* [N] += 1 (may be NULL) */
    float* targets;          /* [N,D] out: clamped PD targets == action_manager.get_actions() */
    GfStepStats* stats;      /* may be NULL */
    GfStepStats* stats_zero; /* optional: GF_STATS_SHARDS blocks this launch zeroes — the NEXT step's slot of a statistics
                                ring, so a recorded step needs neither a memset nor a per-step device→host copy */
    const GfStepStats* stats_fold_src; /* optional: the PREVIOUS step's slot (complete by stream order) … */
    double* stats_fold_dst;            /* … folded over its shards into this GF_STATS_VECTOR_LEN row (layout of gf_stats_pack) */
    double* stats_last_reset;          /* optional: copy of the most recent folded row whose reset_count > 0
                                          (RewardManager.last_episode_mean_reward, reward_manager.py:138-153) */
} GfActionArgs;

/* ------------------------------------------------------------------------------------------
 * Phase B2 — ContactManager.step
 *   managers/contact/kernel.py:5-90 (accumulation), contact_manager.py:384-477 (sanitise, air time)
 * ---------------------------------------------------------------------------------------- */
typedef struct GfContactArgs {
    int32_t num_envs;
    int32_t num_contacts;     /* C */
    int32_t num_scene_links;  /* second dim of links_quat */
    int32_t num_targets;      /* L */
    int32_t num_with;         /* W */
    int32_t has_with_filter;
    int32_t track_air_time;
    int32_t _pad;
    const float* force;       /* [N,C,3] world frame, force on link_b */
    const float* position;    /* [N,C,3] */
    const int32_t* link_a;    /* [N,C] */
    const int32_t* link_b;    /* [N,C] */
    const float* links_quat;  /* [N,num_scene_links,4] */
    const float* links_vel;   /* [N,num_scene_links,3] world link velocities, or NULL */
    float* link_vel_out;      /* [N,L,3] out: velocity of each tracked link (what rewards.feet_slide reads, rewards.py:496-504), or NULL */
    const float* links_pos;   /* [N,num_scene_links,3] world link positions, or NULL */
    float* link_pos_out;      /* [N,L,3] out: position of each tracked link (gait foot_height_reward), or NULL */
    int32_t target_link_ids[GF_MAX_LINK_IDS];
    int32_t with_link_ids[GF_MAX_LINK_IDS];
    float air_time_threshold; /* (float)air_time_contact_threshold */
    float dt;                 /* (float)scene.dt */
    float* contacts;          /* [N,L,3] out */
    float* contact_positions; /* [N,L,3] out (mean position) */
    float* position_counts;   /* [N,L]   out */
    float* last_air_time;     /* [N,L] in/out, NULL unless track_air_time */
    float* current_air_time;
    float* last_contact_time;
    float* current_contact_time;
    GfStepStats* stats;       /* may be NULL */
} GfContactArgs;

/* ------------------------------------------------------------------------------------------
 * Phase B3 — TerminationManager.step   (managers/termination_manager.py:151-190,
 *                                        mdp/terminations.py)
 * ---------------------------------------------------------------------------------------- */
enum {
    GF_T_TIMEOUT = 1,              /* episode_length > max_episode_length          (terminations.py:17-23)  */
    GF_T_BAD_ORIENTATION = 2,      /* p0 = tilt threshold in sin-space, i0 = grace  (terminations.py:26-71)  */
    GF_T_BASE_HEIGHT_BELOW = 3,    /* p0 = minimum height                           (terminations.py:74-99)  */
    GF_T_OUT_OF_BOUNDS = 4,        /* p0..p3 = xmin,xmax,ymin,ymax incl. margin     (terminations.py:102-137)*/
    GF_T_HAS_CONTACT = 5,          /* i0 = contact view, p0 = thr, i1 = min_contacts (terminations.py:139-155)*/
    GF_T_CONTACT_FORCE = 6,        /* i0 = contact view, p0 = thr                   (terminations.py:158-172)*/
    GF_T_CONTACT_FORCE_GRACE = 7,  /* i0 = view, p0 = thr, i1 = grace steps         (terminations.py:175-205)*/
    GF_T_EXTERNAL = 8              /* i0 = ext slot (bool column evaluated by the host) */
};
#define GF_SPAWN_BLOCK 0x100000u  /* Philox counter block of the spawn draws: (x, y, rot z, -) and, in the next block, (rot x, rot y, -, -) */
#define GF_TERM_FLAG_TIME_OUT 1    /* TerminationConfigItem.time_out → OR into truncated */

typedef struct GfTerminationArgs {
    int32_t num_envs;
    int32_t num_terms;
    GfEntityView entity;
    const int32_t* episode_length;
    const int32_t* max_episode_length;  /* may be NULL → timeout never fires */
    GfContactView contact[GF_MAX_CONTACT_VIEWS];
    const uint8_t* ext[GF_MAX_EXT];
    uint8_t* terminated;   /* [N] out */
    uint8_t* truncated;    /* [N] out */
    uint8_t* term_out;     /* [K,N] optional: raw per-term masks (direct mdp.* calls) */
    GfStepStats* stats;    /* may be NULL */
    GfTerm terms[GF_MAX_TERM_TERMS];
} GfTerminationArgs;

/* ------------------------------------------------------------------------------------------
 * Phase B4 — RewardManager.step   (managers/reward_manager.py:166-195, mdp/rewards.py)
 * ---------------------------------------------------------------------------------------- */
enum {
    GF_R_IS_ALIVE = 1,           /* rewards.py:31-37  */
    GF_R_TERMINATED = 2,         /* rewards.py:40-46  */
    GF_R_BASE_HEIGHT = 3,        /* p0 = target | i0 = command view (flag CMD); flag TERRAIN: minus the terrain height under the base  rewards.py:54-90 */
    GF_R_DOF_SIMILAR_TO_DEFAULT = 4, /* rewards.py:93-109  */
    GF_R_LIN_VEL_Z_L2 = 5,       /* rewards.py:112-135 */
    GF_R_ANG_VEL_XY_L2 = 6,      /* rewards.py:138-161 */
    GF_R_FLAT_ORIENTATION_L2 = 7,/* rewards.py:164-193 */
    GF_R_BODY_ACCEL_EXP = 8,     /* p0 = sensitivity, i0 = state slot, flag FIRST_CALL  rewards.py:196-249 */
    GF_R_ACTION_RATE_L2 = 9,     /* rewards.py:257-271 */
    GF_R_CMD_TRACK_LIN_VEL = 10, /* i0 = command view, p0 = sensitivity   rewards.py:279-317 */
    GF_R_CMD_TRACK_ANG_VEL = 11, /* i0 = command view, i1 = column, p0 = sensitivity  rewards.py:320-358 */
    GF_R_STAND_STILL = 12,       /* i0 = command view, p0 = command threshold  rewards.py:361-385 */
    GF_R_HAS_CONTACT = 13,       /* i0 = contact view, p0 = thr, i1 = min_contacts  rewards.py:393-410 */
    GF_R_CONTACT_FORCE = 14,     /* i0 = contact view, p0 = thr   rewards.py:413-428 */
    GF_R_FEET_AIR_TIME = 15,     /* i0 = contact view, i1 = command view or -1, p0 = time_threshold, p1 = max-thr (flag MAX), p2 = (float)(dt+1e-8)  rewards.py:431-469 */
    GF_R_FEET_SLIDE = 16,        /* i0 = contact view  rewards.py:472-504 */
    GF_R_EXTERNAL = 17,          /* i0 = ext slot ([N] f32 column evaluated by the host) */
    /* GaitCommandManager rewards (examples/gait_trainer/gait_command_manager.py:278-345): i0 = contact view of the feet
     * (contacts, link_vel, link_pos), i1 = command view of the gait state rows (GF_GAIT_* columns), i2 = the row of each foot
     * (FL, FR, RL, RR) inside that contact view, one byte each */
    GF_R_GAIT_PHASE = 18,        /* exp(Σ_feet swing ? -|F| : stance ? -|v| : 0)                 :295-345
                                  * Reference quirk reproduced when GfRewardArgs.gait_wave_flags is set: the reference builds its index
                                  * lists with `mask.nonzero().flatten()` on an [N,1] mask (:335-338), which interleaves the COLUMN
                                  * indices (all 0) with the row indices — so env 0 gets the stance weights of a foot whenever ANY
                                  * env is in stance for it, else the swing weights whenever any env is in swing. */
    GF_R_FOOT_HEIGHT = 19        /* exp(-Σ_feet |v_xy| (z - foot_height)^2 / p0), p0 = sensitivity  :278-293 */
};
#define GF_RW_FLAG_CMD 1         /* base_height: target from command view i0 column 0 */
#define GF_RW_FLAG_TERRAIN 2     /* base_height: subtract get_terrain_height(pos.x, pos.y) sampled from GfRewardArgs.terrain */
#define GF_RW_FLAG_MAX 4         /* feet_air_time: clamp max */
#define GF_RW_FLAG_FIRST_CALL 8  /* body_acceleration_exp: no prev state yet */

enum { GF_REWARD_MODE_STEP = 0, GF_REWARD_MODE_EVAL = 1 };

typedef struct GfRewardArgs {
    int32_t num_envs;
    int32_t num_dofs;
    int32_t num_terms;
    int32_t mode;              /* GF_REWARD_MODE_* */
    float dt;                  /* (float)env.dt, added to episode_seconds */
    int32_t logging_enabled;
    GfEntityView entity;
    const float* dof_pos;          /* [N,D] */
    const float* default_dof_pos;  /* [D]   */
    const float* actions;          /* [N,D] raw env.actions      */
    const float* last_actions;     /* [N,D] raw env.last_actions */
    const uint8_t* terminated;     /* [N] extras["terminations"] */
    GfContactView contact[GF_MAX_CONTACT_VIEWS];
    GfCommandView command[GF_MAX_COMMAND_VIEWS];
    const float* ext[GF_MAX_EXT];
    float* state[4];           /* body_acceleration_exp prev (lin,ang) body-frame velocities, [N,6] each */
    float* reward;             /* [N]   out (STEP) */
    float* episode_sums;       /* [T,N] in/out (STEP, logging) */
    float* episode_seconds;    /* [N]   in/out (STEP) */
    float* term_out;           /* [T,N] out (EVAL): unweighted term values */
    GfTerrainView terrain;     /* base_height(terrain_manager=…): sampled in the kernel (rewards.py:84-88) */
    const uint8_t* gait_wave_flags; /* GfGaitArgs.wave_flags of the gait manager GF_R_GAIT_PHASE reads (env-0 quirk), or NULL */
    GfTerm terms[GF_MAX_TERMS];
} GfRewardArgs;

/* ------------------------------------------------------------------------------------------
 * Phase B5 — CommandManager.step / reset / resample_command
 *   managers/command/command_manager.py:152-170,290-303
 * ---------------------------------------------------------------------------------------- */
enum { GF_CMD_STEP = 0, GF_CMD_MASKED = 1, GF_CMD_ALL = 2 };

typedef struct GfCommandArgs {
    int32_t num_envs;
    int32_t num_ranges;       /* R */
    int32_t mode;             /* GF_CMD_* */
    int32_t resample_steps;   /* int(resample_time_sec/dt) */
    const int32_t* episode_length; /* STEP */
    const uint8_t* mask;      /* MASKED: resample where mask!=0 */
    const uint8_t* mask2;     /* MASKED: optional second mask OR-ed in (terminated|truncated) */
    const float* draws;       /* [N,R] U[0,1) or NULL → Philox */
    uint64_t seed;
    uint64_t stream;          /* distinct per (manager, call) so draws never repeat */
    uint32_t env_offset;      /* global index of local env 0 (env sharding): Philox is keyed by the GLOBAL env id */
    uint32_t _pad2;
    float lo[GF_MAX_RANGES];
    float hi[GF_MAX_RANGES];
    float* command;           /* [N,R] in/out */
    GfStepStats* stats;       /* may be NULL (STEP mode counts resamples) */
} GfCommandArgs;

/* ------------------------------------------------------------------------------------------
 * Phase B5' — GaitCommandManager.step / reset / resample_command
 *   examples/gait_trainer/gait_command_manager.py:185-255,347-399 (a user-level CommandManager in the reference's
 *   gait_trainer example).  State of one env = one 64-byte row:
 *     [0..3] foot_offset (FL,FR,RL,RR)  [4] foot_height  [5] gait_period  [6..13] clock_input (4 sin, 4 cos)
 *     [14] gait_time  [15] gait_phase
 *   so columns 0..13 are exactly `observation()` (:257-268) and 0..5 are `command` (:127-141).
 *   STEP  : resample where episode_length % resample_steps == 0 (command_manager.py:152-162), count envs per gait
 *           (_log_metrics, :430-441), then advance the clock for EVERY env (:231-239):
 *             gait_time = fmod(gait_time + dt, period); gait_phase = gait_time / period;
 *             clock[i] = sin(2π·fmod(phase + offset_i, 1)), clock[4+i] = cos(…)
 *   MASKED / ALL : resample the masked envs, zero their clock_input / gait_time / gait_phase (:241-255).
 *   Resampling (:185-211,347-399): gait g from the categorical distribution `cum_weight` (inverse CDF of draw 0; with one
 *   gait no draw is consumed), foot offsets from the gait table, foot_height = clearance_lo for the fixed-clearance gaits
 *   else U(clearance) from draw 1, gait_period = U(period) from draw 2.
 * ---------------------------------------------------------------------------------------- */
enum { GF_GAIT_OFFSET = 0, GF_GAIT_HEIGHT = 4, GF_GAIT_PERIOD = 5, GF_GAIT_CLOCK = 6, GF_GAIT_TIME = 14, GF_GAIT_PHASE = 15,
       GF_GAIT_ROW = 16, GF_GAIT_OBS_WIDTH = 14 };

typedef struct GfGaitArgs {
    int32_t num_envs;
    int32_t mode;               /* GF_CMD_STEP / GF_CMD_MASKED / GF_CMD_ALL */
    int32_t resample_steps;
    int32_t num_gaits;          /* gaits currently sampled from (curriculum), 1..GF_MAX_GAITS */
    const int32_t* episode_length; /* STEP */
    const uint8_t* mask;        /* MASKED */
    const uint8_t* mask2;       /* MASKED, optional */
    const float* draws;         /* [N,3] U[0,1) (gait select, foot clearance, gait period) or NULL → Philox */
    uint64_t seed;
    uint64_t stream;
    uint32_t env_offset;
    int32_t fixed_clearance_mask; /* bit g: gait g always uses clearance_lo ("pronk", "bound"; :366-368) */
    float cum_weight[GF_MAX_GAITS];   /* f32 cumulative sum of the normalised gait weights (:379-399) */
    float gait_offsets[GF_MAX_GAITS][4];
    float clearance_lo, clearance_hi; /* _foot_clearance_range */
    float period_lo, period_hi;       /* _gait_period_range */
    float dt;                   /* (float)env.dt */
    float two_pi;               /* (float)(2*pi) */
    float* state;               /* [N,GF_GAIT_ROW] in/out */
    int64_t* selected;          /* [N] in/out: _gait_selected */
    uint8_t* wave_flags;        /* [ceil(N/64) rounded up to 4] out, optional: for each block of 64 envs, bit 2f = some env of the
                                   block has foot f in swing, bit 2f+1 = in stance, for the CURRENT state (phi = fmod(phase +
                                   offset_f, 1)·2π; swing: 0 <= phi < π, stance: π <= phi < 2π).  Every launch that changes an env
                                   rewrites its block's byte from the 64 rows it holds: no atomics, nothing incremental.  The
                                   host initialises it for the all-zero state (every foot in swing: 0x55). */
    GfStepStats* stats;         /* STEP: gait_count[] += envs per gait; may be NULL */
} GfGaitArgs;

/* ------------------------------------------------------------------------------------------
 * Phase R — masked reset of all manager-owned state (ManagedEnvironment.reset fan-out)
 *   managed_env.py:336-371; genesis_env.py:207-254; reward_manager.py:197-222;
 *   contact_manager.py:316-329; position_action_manager.py:421-464; mdp/reset.py:67-124
 * The reference compacts done envs with nonzero() and gathers/scatters; this is the same
 * update expressed as a mask so no host sync is needed.
 * ---------------------------------------------------------------------------------------- */
typedef struct GfResetArgs {
    int32_t num_envs;
    int32_t num_dofs;
    int32_t num_reward_terms;   /* rows of episode_sums */
    int32_t num_contact;        /* contact managers with air-time state */
    const uint8_t* mask;        /* [N] reset where mask|mask2 != 0 */
    const uint8_t* mask2;       /* optional */
    /* GenesisEnv.reset */
    float* env_actions;         /* [N,D] → 0 */
    float* env_last_actions;    /* [N,D] → 0 */
    int32_t* episode_length;    /* [N]   → 0 */
    int32_t* max_episode_length;/* [N]   → round(base + (2u-1)*max_random_scaling) when scaling>0 */
    int32_t base_max_episode_length;
    float max_random_scaling;   /* (float)(base*max_episode_random_scaling); 0 disables */
    const float* len_draws;     /* [N] U[0,1) or NULL → Philox */
    /* RewardManager.reset */
    float* episode_sums;        /* [T,N] */
    float* episode_seconds;     /* [N] → 1e-10 */
    uint32_t reward_log_mask;   /* bit t set: term t has weight != 0 → value/=secs, accumulate mean */
    int32_t reward_logging;     /* logging_enabled */
    /* ContactManager.reset: 4 air-time arrays per manager */
    float* air_state[GF_MAX_CONTACT_VIEWS][4];
    int32_t air_links[GF_MAX_CONTACT_VIEWS];
    /* Scene-side state, only when the scene exposes masked setters (synthetic scene).
     * NULL pointers skip the section (real Genesis: host calls the envs_idx setters). */
    float* scene_dof_pos;       /* [N,D] ← default_dof_pos + (2u-1)*noise_scale */
    float* scene_dof_vel;       /* [N,D] ← 0 */
    const float* default_dof_pos; /* [D] */
    float dof_noise_scale;
    const float* dof_draws;     /* [N,D] U[0,1) or NULL → Philox (only read when noise_scale != 0) */
    float* scene_pos;           /* [N,3] ← reset_pos    (mdp.reset.position) */
    float* scene_quat;          /* [N,4] ← reset_quat; 16-byte aligned (a row moves as one unit), else GF_E_UNSUPPORTED */
    float* quat_stash;          /* [N,4] optional: receives the pre-reset quat of every reset env (see GfObservationArgs.stale_quat);
                                   16-byte aligned when scene_quat is set, else GF_E_UNSUPPORTED */
    float* scene_lin_vel;       /* [N,3] ← 0 when zero_velocity */
    float* scene_ang_vel;       /* [N,3] ← 0 when zero_velocity */
    float reset_pos[3];
    float reset_quat[4];
    int32_t set_quat;
    int32_t zero_velocity;
    uint64_t seed;
    uint64_t stream;
    uint32_t env_offset;        /* global index of local env 0 */
    /* mdp.reset.randomize_terrain_position (mdp/reset.py:127-226 → terrain_manager.py:170-279): with spawn_mode = 1 the base of a
     * reset env goes to x = u0*spawn_x_span + spawn_x_min, y = u1*spawn_y_span + spawn_y_min (the usable centre area),
     * z = terrain height there + spawn_height_offset, instead of reset_pos; with spawn_set_quat = 1 its orientation becomes
     * xyz_to_quat(rx, ry, rz) where axis k is U(spawn_rot_lo[k], spawn_rot_hi[k]) if bit k of spawn_rot_mask is set and 0
     * otherwise (define_quat only writes the axes given as (lo, hi) tuples, reset.py:172-196; default {"z": (0, 2π)}). */
    int32_t spawn_mode;
    int32_t spawn_set_quat;
    int32_t spawn_rot_mask;
    float spawn_x_min, spawn_x_span;
    float spawn_y_min, spawn_y_span;
    float spawn_height_offset;
    float spawn_rot_lo[3], spawn_rot_hi[3];
    const float* spawn_draws;   /* [N,5] U[0,1) (x, y, rot x, rot y, rot z) or NULL → Philox blocks GF_SPAWN_BLOCK, +1 of `stream` */
    GfTerrainView terrain;
    GfStepStats* stats;         /* may be NULL */
} GfResetArgs;

/* ------------------------------------------------------------------------------------------
 * Phase O — ObservationManager.get_observations
 *   managers/observation_manager.py:218-256, mdp/observations.py
 * ---------------------------------------------------------------------------------------- */
enum {
    GF_O_COMMAND = 1,          /* i0 = command view; width = view width */
    GF_O_ANG_VEL_BODY = 2,     /* EntityManager.get_angular_velocity  (entity_manager.py:142-146) */
    GF_O_LIN_VEL_BODY = 3,     /* EntityManager.get_linear_velocity   (entity_manager.py:136-140) */
    GF_O_PROJ_GRAVITY = 4,     /* EntityManager.get_projected_gravity (entity_manager.py:130-134) */
    GF_O_DOF_POS = 5,          /* action_manager.get_dofs_position()  */
    GF_O_DOF_VEL = 6,          /* action_manager.get_dofs_velocity()  */
    GF_O_DOF_FORCE = 7,        /* action_manager.get_dofs_force()     */
    GF_O_ACTIONS = 8,          /* action_manager.get_actions() == clamped targets (quirk q1) */
    GF_O_RAW_ACTIONS = 9,      /* env.actions */
    GF_O_CONTACT_FORCE_NORM = 10, /* i0 = contact view; width = L  (observations.py:182-193) */
    GF_O_EXTERNAL = 11,        /* i0 = ext slot, i1 = width: [N,width] f32 evaluated by the host */
    GF_O_BASE_POS = 12,
    GF_O_BASE_QUAT = 13
};

typedef struct GfObsItem {
    int32_t op;
    int32_t width;
    int32_t i0;
    int32_t i1;
    float scale;   /* ObservationConfigItem.scale (1.0 = none) */
    float noise;   /* item noise or manager noise; 0 = none     */
} GfObsItem;

typedef struct GfObservationArgs {
    int32_t num_envs;
    int32_t num_dofs;
    int32_t num_items;
    int32_t obs_width;        /* O = Σ width */
    int32_t history_len;      /* H >= 1 */
    int32_t history_ring;     /* 0: `obs` = [new frame | the first H-1 frames of prev_obs] (newest first, observation_manager.py:218-226:
                                 the previous OUTPUT is the history, so a launch moves (2H-1)·O floats per env);
                                 k+1: IN-PLACE RING — `obs` is the persistent [N, H, O] history itself and the launch writes ONLY the new
                                 frame, into frame slot k (0 <= k < H); prev_obs is unused.  O floats per env instead of (2H-1)·O; the
                                 caller walks the slots from k upwards (wrapping) to read newest first: the host passes
                                 k = (H - step % H) % H so that this walk is ascending in memory. */
    GfEntityView entity;
    const float* dof_pos;     /* [N,D] */
    const float* dof_vel;     /* [N,D] */
    const float* dof_force;   /* [N,D] */
    const float* targets;     /* [N,D] */
    const float* env_actions; /* [N,D] */
    GfContactView contact[GF_MAX_CONTACT_VIEWS];
    GfCommandView command[GF_MAX_COMMAND_VIEWS];
    const float* ext[GF_MAX_EXT];
    const float* noise_draws; /* [N,O] U[0,1) or NULL → Philox */
    uint64_t seed;
    uint64_t stream;
    uint32_t env_offset;      /* global index of local env 0 */
    uint32_t ring_slots;      /* history_ring != 0 only.  0: the ring has history_len frame slots (`obs` = [N, H, O]).  S >= history_len: `obs` is
                                 [N, S, O] — the env stride is S·O floats — and history_ring - 1 < S.  With more slots than frames the host can
                                 hand out H consecutive slots as a newest-first WINDOW of the buffer (a strided view, no gather): it walks the
                                 slot downwards and mirrors the newest H-1 frames behind slot S' when the walk wraps
                                 (ObservationManager output="window").  (This word was padding before: 0 = the old behaviour.) */
    /* The reference's EntityManager caches base_quat at entity.step() and does not refresh it after the reset
     * that follows in the same tick (entity_manager.py:163-167,189-195): body-frame items of envs that were just
     * reset are rotated by their PRE-reset quaternion.  stale_quat (written by gf_masked_reset.quat_stash) supplies
     * it for envs whose stale_mask|stale_mask2 byte is set; NULL disables. */
    const float* stale_quat;  /* [N,4] */
    const uint8_t* stale_mask;
    const uint8_t* stale_mask2;
    const float* prev_obs;    /* [N,O*H] previous output (history shift source); NULL when H==1 */
    float* obs;               /* [N,O*H] out, newest frame first (observation_manager.py:224-226) */
    GfObsItem items[GF_MAX_OBS_ITEMS];
} GfObservationArgs;

/* ------------------------------------------------------------------------------------------
 * Entity helpers — EntityManager.get_projected_gravity / get_linear_velocity /
 * get_angular_velocity as standalone calls (entity_manager.py:130-146; utils.py:13-55).
 * ---------------------------------------------------------------------------------------- */
enum { GF_ROT_PROJ_GRAVITY = 0, GF_ROT_LIN_VEL = 1, GF_ROT_ANG_VEL = 2 };
typedef struct GfRotateArgs {
    int32_t num_envs;
    int32_t what;         /* GF_ROT_* */
    GfEntityView entity;
    float* out;           /* [N,3] */
} GfRotateArgs;

/* ------------------------------------------------------------------------------------------
 * TerrainManager.get_terrain_height (managers/terrain_manager.py:100-166): bilinear sample of the shared
 * height field at world (x, y), `F.grid_sample(mode="bilinear", padding_mode="border", align_corners=True)`:
 *   nx = ((x - x_min) / x_span) * 2 - 1            (the in-place chain of :123-136, one rounding per op)
 *   ix = clamp(((nx + 1) / 2) * (W - 1), 0, W - 1) (unnormalise + border clip), same for iy with H
 *   out = nw*v[y0,x0] + ne*v[y0,x1] + sw*v[y1,x0] + se*v[y1,x1], weights (x1-ix)(y1-iy) …, taps outside the field
 *   contribute nothing (only x1 = W / y1 = H, where the weight is 0 anyway).
 * x and y are strided so `pos[:, 0]`, `pos[:, 1]` of an [N,3] tensor (rewards.py:85-87) or columns of the spawn
 * buffer (terrain_manager.py:236-239) are read in place.
 * ---------------------------------------------------------------------------------------- */
typedef struct GfTerrainHeightArgs {
    int64_t num;           /* number of queries */
    const float* x;        /* element i at x[i * x_stride] */
    const float* y;
    int64_t x_stride;      /* in floats */
    int64_t y_stride;
    GfTerrainView terrain;
    float* out;            /* [num] */
} GfTerrainHeightArgs;

/* ------------------------------------------------------------------------------------------
 * Synthetic scene tick — stands in for Genesis' scene.step() in benchmarks and parity tests
 * (SURVEY.md §7 step 5).  Deterministic, integer-Philox driven, f32 ops in a fixed order so the
 * HIP kernel, the C oracle and the numpy model used to drive the reference agree bit for bit.
 * ---------------------------------------------------------------------------------------- */
typedef struct GfSynthSceneArgs {
    int32_t num_envs;
    int32_t num_dofs;
    int32_t num_contacts;     /* C (0: no contact generation) */
    int32_t num_scene_links;
    float dt;
    float joint_rate;         /* first-order tracking gain [1/s] */
    float ang_noise;          /* rad/s per tick */
    float lin_noise;          /* m/s per tick */
    float height_target;
    float contact_prob;       /* per slot (walking model: per BODY slot) */
    float contact_force;      /* force scale */
    float foot_contact_prob;  /* walking model (foot_link_mask != 0): mean per-tick probability that a foot touches the ground */
    const float* targets;     /* [N,D] PD targets written by phase A */
    float* pos;               /* [N,3] in/out */
    float* quat;              /* [N,4] in/out */
    float* lin_vel;           /* [N,3] in/out */
    float* ang_vel;           /* [N,3] in/out */
    float* dof_pos;           /* [N,D] in/out */
    float* dof_vel;           /* [N,D] out    */
    float* contact_force_out; /* [N,C,3] or NULL */
    float* contact_pos_out;   /* [N,C,3] */
    int32_t* link_a_out;      /* [N,C] */
    int32_t* link_b_out;      /* [N,C] */
    float* links_quat_out;    /* [N,num_scene_links,4] */
    float* links_vel_out;     /* [N,num_scene_links,3] or NULL */
    float* links_pos_out;     /* [N,num_scene_links,3] or NULL: world position of every link (RigidEntity.get_links_pos) */
    uint64_t seed;
    uint64_t tick;
    uint32_t env_offset;      /* global index of local env 0 */
    /* Walking contact model.  0: every slot is an independent (ground, random robot link) contact with probability contact_prob.
     * Otherwise bit l marks scene link l (< 32) as a FOOT: the k-th foot owns slot k — its contact with the ground, made with
     * probability min(1, 1.8 p) while the foot is in the stance half of a 20-tick trot cycle (diagonal pairs alternate, the
     * cycle offset differs per env) and 0.2 p in the swing half, p = foot_contact_prob (its normal force comes from the draw that picks the side): two to four feet of a quadruped on the
     * ground every tick, as the reference's foot ContactManager / feet_air_time / the Taichi kernel's matching branch expect
     * (examples/gait_trainer/environment.py:140-153, mdp/rewards.py:431-469, managers/contact/kernel.py:47-78).  The remaining
     * slots are body contacts as before (probability contact_prob, any robot link).  Every contact puts the ground on side a or
     * side b at random (force stored as the force on link_b, so it is negated when the robot link is link_a): both branches of
     * kernel.py:74-78 run. */
    uint32_t foot_link_mask;
} GfSynthSceneArgs;

/* ------------------------------------------------------------------------------------------
 * Rollout storage write (first slice): what the RL library does with a step's outputs.
 * rsl_rl's OnPolicyRunner (call site examples/simple/train.py:125-129, `num_steps_per_env` = 24, :75) copies every
 * step's observation, reward and done flags into a time-major RolloutStorage with three `copy_` launches
 * (`observations[step].copy_(obs)`, `rewards[step].copy_(rew)`, `dones[step].copy_(dones)`).  Here the step's own
 * kernel stores them: the fused post-physics launch writes its observation tile, reward and masks a second time,
 * straight into the storage rows (GfPostRefs.rollout), or gf_rollout_write does it as one launch.
 * Layout (plain pointers, time-major, contiguous): observations [T+1, N, W] f32, rewards [T, N] f32, dones [T, N] u8.
 * Step t of a rollout writes rewards[t], dones[t] = terminated | truncated, and observations[t+1] = the observation the
 * step RETURNS (the policy's next input; row T is the bootstrap observation, row 0 the one the rollout started from).
 * The caller passes the row addresses, so the library needs neither T nor t.
 * ---------------------------------------------------------------------------------------- */
typedef struct GfRolloutArgs {
    int32_t num_envs;
    int32_t obs_width;          /* W: floats per env of `obs` (O·H of the policy ObservationManager) */
    const float* obs;           /* [N, W] the observation this step returns */
    const float* reward;        /* [N] */
    const uint8_t* terminated;  /* [N] */
    const uint8_t* truncated;   /* [N] */
    float* obs_out;             /* &observations[t+1][0][0], or NULL */
    float* reward_out;          /* &rewards[t][0], or NULL */
    uint8_t* done_out;          /* &dones[t][0], or NULL */
} GfRolloutArgs;

/* ------------------------------------------------------------------------------------------
 * The newest frame of a history observation into a frame-major rollout storage (learner.RolloutStorage(history="frames")).
 * The reference's observation history is a pure sliding window (observation_manager.py:218-226: pop, insert(0, obs), cat — never
 * cleared per env, untouched by a reset), so the [N, H·O] row a step returns is frames t, t-1 … t-H+1 and a storage that keeps
 * every FRAME once — frames [T + H, N, O] — holds every row: observation row r is frames r … r+H-1, frame r+H-1 the newest.
 * A step then stores O floats per env instead of H·O.  gf_rollout_frame_write copies, for up to GF_ROLLOUT_FRAME_MAX managers in
 * ONE launch,
 *     segs[s].dst[n * width + c] = segs[s].src[n * src_stride + c]        (n < num_envs, c < width)
 * `src` is the tensor the step returned (newest frame first: columns 0 … O-1), `src_stride` its row stride in floats — H·O for a
 * contiguous row, the slot stride of an output="window" view.  Chunks of 16, 8 or 4 bytes, chosen per segment from the alignment of
 * src, dst, width and src_stride.  Pure copy.  Algorithmic traffic: R 4·O, W 4·O bytes per env and segment.
 * Refusals, before anything is launched: GF_E_NULL — args, a src / dst pointer; GF_E_RANGE — num_envs < 0, num_segs outside
 * 1 … GF_ROLLOUT_FRAME_MAX, width < 1, src_stride < width.  num_envs == 0 is a no-op.  Not a phase of the step: it never enters a
 * recorded step's op table (the storage issues it right behind the step's gf_rollout_write).
 * ---------------------------------------------------------------------------------------- */
#define GF_ROLLOUT_FRAME_MAX 4

typedef struct GfRolloutFrameSeg {
    const float* src;           /* [N, >= width] rows src_stride floats apart: the newest frame is columns 0 … width-1 */
    float* dst;                 /* [N, width] contiguous: &frames[t + H][0][0] */
    int32_t width;              /* O >= 1 */
    int32_t src_stride;         /* >= width, in floats */
} GfRolloutFrameSeg;

typedef struct GfRolloutFrameArgs {
    int64_t num_envs;           /* N >= 0; 0: nothing is launched */
    int32_t num_segs;           /* 1 … GF_ROLLOUT_FRAME_MAX */
    int32_t _pad;
    GfRolloutFrameSeg segs[GF_ROLLOUT_FRAME_MAX];
} GfRolloutFrameArgs;

/* ------------------------------------------------------------------------------------------
 * The policy's half of a transition and the return computation (remainder).  rsl_rl's OnPolicyRunner
 * (third-party; configured and called by the reference at examples/simple/train.py:37-79,125-129: PPO, gamma 0.99, lam 0.95,
 * num_steps_per_env 24) stores, besides the env's outputs, what the policy produced for the step — actions, value estimate,
 * log-probability, action mean and std: five more `copy_` launches in RolloutStorage.add_transitions — after bootstrapping
 * time-outs into the reward (PPO.process_env_step: rewards += gamma * values * time_outs), and at the end of a rollout runs
 * RolloutStorage.compute_returns: a loop over the T steps, backwards, of eight elementwise launches each (GAE, Schulman et
 * al. 2016), then normalises the advantages — ~200 launches for T = 24.
 *   gf_rollout_policy_write: the five rows and the time-out bootstrap in ONE launch.
 *   gf_gae:  for each env (one lane; rows of the time-major arrays are read and written coalesced), t = T-1 … 0:
 *       next  = t == T-1 ? last_values[n] : values[t+1][n];   live = 1 - dones[t][n]
 *       delta = rewards[t][n] + live * gamma * next - values[t][n]
 *       adv   = delta + live * gamma * lam * adv;            returns[t][n] = adv + values[t][n]
 *     advantages[t][n] = returns[t][n] - values[t][n]; with `normalize`, a second launch maps them to
 *     (adv - mean) / (std + 1e-8) over all T*N entries (unbiased std, as torch.std), from f64 moments the first launch
 *     accumulates (one atomic pair per wave).  One f32 operation per step of the recurrence in this order: bit-identical
 *     to the torch loop before normalisation.  Algorithmic traffic: R 9 + W 8 bytes per (step, env) (+ R/W 8 to normalise).
 * ---------------------------------------------------------------------------------------- */
typedef struct GfRolloutPolicyArgs {
    int32_t num_envs;
    int32_t num_actions;        /* A */
    const float* actions;       /* [N, A] sampled actions, or NULL (each source may be NULL together with its row) */
    const float* values;        /* [N] value estimates */
    const float* log_prob;      /* [N] */
    const float* mu;            /* [N, A] action mean */
    const float* sigma;         /* [N, A] action std */
    float* actions_out;         /* &actions[t][0][0] of the time-major storage */
    float* values_out;          /* &values[t][0] */
    float* log_prob_out;        /* &actions_log_prob[t][0] */
    float* mu_out;              /* &mu[t][0][0] */
    float* sigma_out;           /* &sigma[t][0][0] */
    const uint8_t* time_outs;   /* [N] truncated flags of this step, or NULL: reward_row[n] += gamma * values[n] * time_outs[n] */
    float* reward_row;          /* &rewards[t][0] (read-modify-write), required with time_outs */
    float gamma;
    int32_t _pad;
} GfRolloutPolicyArgs;

typedef struct GfGaeArgs {
    int32_t num_envs;
    int32_t num_steps;          /* T >= 1 */
    const float* rewards;       /* [T, N] */
    const float* values;        /* [T, N] */
    const uint8_t* dones;       /* [T, N] */
    const float* last_values;   /* [N] value of the bootstrap observation */
    float gamma, lam;
    float* returns;             /* [T, N] */
    float* advantages;          /* [T, N] */
    double* moments;            /* [2] scratch: sum and sum of squares of the advantages; required with normalize */
    int32_t normalize;          /* 1: advantages <- (advantages - mean) / (std + 1e-8) */
    int32_t _pad;
} GfGaeArgs;

/* ------------------------------------------------------------------------------------------
 * The index list of a step's done envs.  The reference compacts `(terminated | truncated).nonzero()` on every step
 * (managed_env.py:308-310) and hands the list to `reset(ids)`; on the masked path nothing needs it — except code that takes
 * index lists by contract: Genesis' `envs_idx` setters (position_action_manager.py:455-464, mdp/reset.py:102-124), a user's
 * `reset(ids)` override, user-defined manager classes.  torch's `nonzero()` there is an OR launch, a two-pass select, a
 * device-to-host copy of the count and an allocation.  gf_done_compact: one small launch up to 131 072 envs (a block counts the masks in front of it itself), two above — per-block counts, then
 * offsets + ordered writes — produce the ascending list in a caller-owned buffer and the count in a word the host reads after
 * synchronising the stream (pinned host memory).  Same order as nonzero(), so everything downstream is unchanged.
 * ---------------------------------------------------------------------------------------- */
typedef struct GfCompactArgs {
    int64_t num_envs;
    const uint8_t* mask;      /* [N] nonzero = listed */
    const uint8_t* mask2;     /* [N] OR-ed in, or NULL */
    int64_t* ids_out;         /* [N] capacity; the first *count_out entries are the indices, ascending */
    int32_t* count_out;       /* one word: device memory or pinned host memory */
    int32_t* block_counts;    /* scratch, ceil(N / 4096) + 1 words */
    int32_t wait;             /* 1: the call returns after the stream has drained — *count_out (pinned host memory) is then valid
                               * for the caller to read: the one synchronisation of a step that needs the list, taken inside the
                               * call instead of through a second trip into the runtime */
    int32_t _pad;
} GfCompactArgs;

/* ------------------------------------------------------------------------------------------
 * PPO minibatches of a finished rollout (rsl_rl RolloutStorage.mini_batch_generator).  rsl_rl draws one permutation of the
 * T·N transitions per call and builds each minibatch by indexing every flattened [T·N, …] array with a slice of it — obs,
 * critic obs, actions, values, advantages, returns, log-prob, mu, sigma: nine index launches that read and write every stored
 * byte once per epoch.  gf_minibatch_gather copies every field of the selected rows in ONE launch:
 *     fields[f].dst[i * dst_width + dst_col + c] = fields[f].src[indices[i] * src_width + c]   (i < num_rows, c < src_width)
 * `dst_col` lets the members of a concatenated observation group land side by side in one [num_rows, dst_width] output.
 * An index outside [0, num_src_rows) is never dereferenced: its row is written as quiet NaN in every field.  Pure copy:
 * bit-identical to `src[indices]` — unless the field carries a normaliser (`mean != NULL`; rsl_rl EmpiricalNormalization.forward
 * on the gathered observations): its elements are then stored as
 *     (src[indices[i], c] - mean[c]) / (std[c] + eps)        (one subtraction, one addition, one correctly rounded division)
 * by the same launch.  `mean` / `std` are `[src_width]`; a member of a concatenated group points at its slice of the group's
 * normaliser (`norm.mean + dst_col`), so the two vectors may be less aligned than the rows: they are read by element.  Rows of
 * out-of-range indices stay quiet NaN.  Refusals: GF_E_NULL — `mean` without `std`.
 * History field (`history_len` = H > 1; 0 or 1: the plain field above): `src` is a frame-major storage [(T + H)·N, O] (O = src_width,
 * N = frame_stride_rows) whose row t·N + n is the OLDEST frame of observation row t of env n; the newer frames lie whole multiples
 * of N rows further on, so no division by N is needed.  The field fills H·O destination columns, newest frame first:
 *     dst[i * dst_width + dst_col + j * O + c] = src[(indices[i] + (H-1-j) * N) * O + c]          (j < H, c < O)
 * The caller guarantees that `src` holds num_src_rows + (H-1)·N rows.  An out-of-range index gives quiet NaN in all H·O columns.
 * With a normaliser, `mean` / `std` span the field's H·O columns (index j·O + c); the arithmetic per element is unchanged.  The
 * chunk width must hold for every frame's address too: frame_stride_rows·src_width enters the alignment test (it is a multiple
 * of the chunk whenever src_width is: O = 78 moves in 8-byte chunks for every N, O = 16 in 16-byte chunks).  Refusals: GF_E_RANGE — history_len < 0, frame_stride_rows < 1 with history_len > 1,
 * dst_col + H·O > dst_width.
 * Not a phase of the step: it never enters a recorded step's op table.
 * ---------------------------------------------------------------------------------------- */
#define GF_MINIBATCH_MAX_FIELDS 12

typedef struct GfMinibatchField {
    const float* src;           /* [num_src_rows, src_width] f32, row-major */
    float* dst;                 /* [num_rows, dst_width] f32, row-major */
    int32_t src_width;          /* >= 1 */
    int32_t dst_width;          /* >= dst_col + max(H, 1) * src_width */
    int32_t dst_col;            /* first destination column of this field */
    int32_t history_len;        /* H; 0 or 1: a plain field.  > 1: `src` holds frames, the field is H * src_width columns wide */
    const float* mean;          /* [max(H, 1) * src_width] normaliser mean, or NULL: pure copy */
    const float* std;           /* [max(H, 1) * src_width] normaliser std (required with mean) */
    float eps;                  /* added to std */
    int32_t frame_stride_rows;  /* N: source rows from a frame to the next newer one (read when history_len > 1; then >= 1) */
} GfMinibatchField;

typedef struct GfMinibatchArgs {
    int64_t num_rows;           /* rows of the minibatch; 0: nothing is launched */
    int64_t num_src_rows;       /* T·N >= 1: indices at or past it (or negative) give NaN rows */
    const int64_t* indices;     /* [num_rows] source rows (a slice of torch.randperm) */
    int32_t num_fields;         /* 1 … GF_MINIBATCH_MAX_FIELDS */
    int32_t _pad;
    GfMinibatchField fields[GF_MINIBATCH_MAX_FIELDS];
} GfMinibatchArgs;

/* ------------------------------------------------------------------------------------------
 * Gaussian action sampling of a PPO collection step (rsl_rl PPO.act -> ActorCritic.act / get_actions_log_prob).  rsl_rl builds
 * Normal(mean, std), samples with torch.normal, computes log_prob(actions).sum(-1) — about ten elementwise launches on [N, A] —
 * and add_transitions then copies the results into the storage.  gf_policy_act does all of it in ONE launch, one lane per env:
 *     eps     = noise[n, a]  or  Philox4x32-10 + Box–Muller (below)
 *     actions = mean + std * eps                                        (one product, one sum: torch.normal's order)
 *     log_prob[n] = left fold over a of  -((act - mean)^2) / (2 * std^2) - log(std) - c,   c = (float)log(sqrt(2π))
 *                                                                       (the operation order of torch's Normal.log_prob)
 * and stores actions into the fresh `actions` tensor and, where given, the storage rows of transition t (actions, mu = mean,
 * sigma = std expanded to [N, A], values, actions_log_prob).
 * std_is_log = 1 (rsl_rl's noise_std_type = "log"): `std` holds log_std and every loaded element e stands for expf(e) — in the
 * sample, in the log_prob fold (logf of the exponentiated value, as torch's scale.log()) and in the sigma row, which holds std,
 * never log_std.  gf_mlp_act and gf_ppo_loss exponentiate by the same code: one log_std gives the same sigma bits in all three.
 * With the flag 0 nothing is exponentiated.  Refusals, before anything is launched: GF_E_NULL — args, mean, std, actions,
 * values_out without values; GF_E_RANGE — num_envs < 0, num_actions < 1, std_per_env or std_is_log outside {0, 1}.
 * Draws: Philox block (env_offset + n, a / 4, stream_lo, stream_hi) keyed by seed ^ GF_POLICY_SEED_TAG (never the env's own key,
 * so no env draw is ever repeated) gives the normals of columns 4k … 4k+3: words (x, y) -> columns 4k, 4k+1 and (z, w) -> 4k+2, 4k+3,
 *     u1 = ((word1 >> 8) + 1) · 2^-24 ∈ (0, 1],  u2 = (word2 >> 8) · 2^-24,  r = sqrt(-2 · log(u1)),
 *     first = r · cospi(2 · u2),  second = r · sinpi(2 · u2).
 * Not a phase of the step: it never enters a recorded step's op table.
 * ---------------------------------------------------------------------------------------- */
#define GF_POLICY_SEED_TAG 0xAC7105A3C7105EEDull   /* XOR-ed into the seed of the action noise: a key of its own */

typedef struct GfPolicyActArgs {
    int64_t num_envs;           /* N >= 0; 0: nothing is launched */
    int32_t num_actions;        /* A >= 1 */
    int32_t std_per_env;        /* 0: std is [A] (shared by every env), 1: std is [N, A] */
    const float* mean;          /* [N, A] actor output */
    const float* std;           /* [A] or [N, A]: the std, or log_std with std_is_log */
    const float* values;        /* [N] critic output, or NULL (then values_out must be NULL) */
    const float* noise;         /* [N, A] standard normals (parity mode), or NULL: Philox + Box–Muller */
    uint64_t seed;              /* Philox key = seed ^ GF_POLICY_SEED_TAG */
    uint64_t stream;            /* Philox counter words 2-3 */
    uint32_t env_offset;        /* global index of local env 0 (env sharding) */
    uint32_t std_is_log;        /* 0: `std` is the std, 1: it is log_std (sigma = expf) */
    float* actions;             /* [N, A] out (required) */
    float* actions_out;         /* [N, A] storage row, or NULL */
    float* mu_out;              /* [N, A] storage row, or NULL */
    float* sigma_out;           /* [N, A] storage row, or NULL */
    float* values_out;          /* [N] storage row, or NULL */
    float* log_prob_out;        /* [N] storage row, or NULL */
} GfPolicyActArgs;

/* ------------------------------------------------------------------------------------------
 * Time-out bootstrap and the episode statistics of rsl_rl's OnPolicyRunner.learn.  Every step the runner does
 *     cur_reward_sum += rewards; cur_episode_length += 1; new_ids = (dones > 0).nonzero()
 *     rewbuffer.extend(cur_reward_sum[new_ids].cpu()...); lenbuffer.extend(cur_episode_length[new_ids].cpu()...)
 *     cur_reward_sum[new_ids] = 0; cur_episode_length[new_ids] = 0
 * (about eight launches and two or three host synchronisations; rewbuffer / lenbuffer are deque(maxlen=window)), and
 * PPO.process_env_step bootstraps the rewards of timed-out envs.  gf_episode_step does both in ONE launch up to
 * GF_EPISODE_SINGLE_MAX envs and in two above (a per-block count of the done envs, then everything else), as gf_done_compact:
 *   * cur_reward_sum[n] += rewards[n] (one f32 add), cur_episode_length[n] += 1;
 *   * every done env appends (cur_reward_sum, cur_episode_length) to the ring in ascending env order, then both are zeroed; the
 *     ring keeps the last `window` entries, like deque.extend: of a step's `count` finished envs, rank k survives iff
 *     k >= count - window, at slot (head + k) mod window.  A block finds the done envs in front of it by counting the masks itself
 *     (one launch) or from the per-block counts (two launches) — no inter-workgroup wait;
 *   * ring_state holds {head, fill} twice: the launch reads slot `parity` and writes slot 1 - parity (a host-side call counter's
 *     parity), so no block ever reads a word another block of the same launch writes;
 *   * with time_outs: rewards[n] = rewards[n] + (gamma * values[n]) * time_out — after the statistics read the raw reward (the
 *     runner counts the reward before the bootstrap), the same expression as gf_rollout_policy_write.
 * Not a phase of the step: it never enters a recorded step's op table.
 * ---------------------------------------------------------------------------------------- */
#define GF_EPISODE_BLOCK_ENVS 1024      /* envs per workgroup (256 lanes x 4) */
#define GF_EPISODE_SINGLE_MAX 65536     /* one launch up to this many envs; above it, two (block_counts required) */

typedef struct GfEpisodeArgs {
    int64_t num_envs;           /* N, 0 <= N < 2^31; 0: nothing is launched */
    float* rewards;             /* [N] raw rewards of the step (required); rewritten in place by the bootstrap */
    const uint8_t* dones;       /* [N] nonzero = done (required with statistics) */
    const uint8_t* time_outs;   /* [N] nonzero = timed out, or NULL: no bootstrap */
    const float* values;        /* [N] value estimates of the transition (required with time_outs) */
    float* cur_reward_sum;      /* [N], or NULL: no statistics (then every statistics pointer is NULL) */
    float* cur_episode_length;  /* [N] */
    float* ring_reward;         /* [window] finished returns */
    float* ring_length;         /* [window] finished lengths */
    int32_t* ring_state;        /* [2][2] {head, fill}: slot `parity` is read, slot 1 - parity written */
    int32_t* block_counts;      /* scratch, ceil(N / GF_EPISODE_BLOCK_ENVS) words: required above GF_EPISODE_SINGLE_MAX envs */
    float gamma;
    int32_t window;             /* ring capacity >= 1 (with statistics) */
    int32_t parity;             /* 0 or 1 */
    int32_t _pad;
} GfEpisodeArgs;

/* ------------------------------------------------------------------------------------------
 * The PPO update (rsl_rl PPO.update, non-recurrent path without RND; the symmetry options have their own block below).  Per minibatch rsl_rl evaluates the policy,
 * builds the loss from a few dozen elementwise and reduction launches (and as many for their backward), clips the gradient
 * norm, takes an Adam step and reads four scalars back to the host (the KL test of the adaptive schedule, three .item()).
 * The MLP forward / backward stay in torch; the rest is two entry points that never synchronise:
 *
 * gf_ppo_loss — value and gradient of the minibatch loss for mb rows and A actions (sigma [A] shared by all rows):
 *     logp_i   = left fold over a of  -((x - mu)^2) / (2 sigma^2) - log(sigma) - c       (Normal.log_prob order, as gf_policy_act)
 *     entropy  = sum_a (0.5 + 0.5 log 2π + log sigma_a)                                  (identical for every row)
 *     kl_i     = sum_a [log(sigma / old_sigma + 1e-5) + (old_sigma^2 + (old_mu - mu)^2) / (2 sigma^2) - 0.5]
 *     ratio_i  = exp(logp_i - old_log_prob_i)
 *     surrogate  = mean_i max(-adv·ratio, -adv·clamp(ratio, 1 - eps, 1 + eps))
 *     value_loss = mean_i max((v - R)^2, (v_c - R)^2),  v_c = target + clamp(v - target, -eps, eps)   (clipped)
 *                  mean_i (R - v)^2                                                                     (otherwise)
 *     loss     = surrogate + value_loss_coef · value_loss - entropy_coef · entropy
 * and d loss / d (mu, value, sigma) as torch autograd gives them (clamp passes the gradient at its bounds, a max tie sends half
 * to each side, the KL carries none).  One lane per row, columns in groups of four (16-byte loads where A % 4 == 0 and every
 * row is 16-byte aligned).  Every workgroup leaves 3 + A double partials (surrogate, value loss and KL sums, then the
 * column sums of grad_sigma) in the caller's workspace; a second, one-workgroup launch sums them in a fixed order and writes
 * grad_sigma, out[] and the running sums.  No float atomics, no hand-off between workgroups: bitwise reproducible.
 * sigma_is_log = 1 (rsl_rl's noise_std_type = "log"): `sigma` points at log_std [A] and sigma_a = expf(log_std_a) — the same code
 * as gf_policy_act's, so the same bits — stands wherever sigma does above.  grad_sigma[a] then receives d loss / d log_std_a =
 * g · sigma_a (exp's backward), g the float32 value the flag-0 call writes for that sigma: one more correctly rounded f32 product.
 * kl_rows (rsl_rl with symmetry augmentation: the minibatch is [originals; mirrored copies] and the KL of the schedule is taken from
 * the original rows): 0 — the KL sum and its divisor cover all mb rows, the bits of a call without the field; 1 … mb — they cover the
 * first kl_rows rows, and old_mu / old_sigma hold kl_rows rows (rows past them are never read); every other output is unchanged.
 * Anything else is GF_E_RANGE.
 *
 * gf_adam_step — torch.nn.utils.clip_grad_norm_ then torch.optim.Adam (defaults: no weight decay, no amsgrad; foreach order)
 * over one flat float32 parameter buffer and its flat gradient (the GradientAllReduce bucket):
 *     adaptive schedule: kl > (float)(2·desired) -> lr = max(1e-5, lr / 1.5);  kl < (float)(desired / 2) and kl > 0 -> lr =
 *                        min(1e-2, lr · 1.5)   (kl the float32 kl_mean; lr in double, as Python)
 *     coef = min(1, max_norm / (||g||_2 + 1e-6));  g *= coef (written back, as clip_grad_norm_ leaves it)
 *     m += (1 - b1)(g - m);  v = v·b2 + (1 - b2)·g·g;  p += (float)(-lr / bc1) · (m / (sqrt(v) / (float)sqrt(bc2) + eps))
 *     with bc1 = 1 - b1^step, bc2 = 1 - b2^step in double.
 * Launch 1 leaves per-workgroup partial sums of g^2 (double) in the workspace; launch 2 has every workgroup sum them in the
 * same order (no hand-off), apply the schedule to state[parity] and update its elements; workgroup 0 writes state[1 - parity]
 * (double-buffered by call parity, as GfEpisodeArgs.ring_state).
 *
 * Neither is a phase of the step.  Refusals (GF_E_NULL / GF_E_RANGE; sigma_is_log outside {0, 1} is GF_E_RANGE) launch nothing;
 * mb == 0 / numel == 0 is a no-op.  No allocation, no copy, no synchronisation inside either entry point.
 * ---------------------------------------------------------------------------------------- */
#define GF_PPO_BLOCK_ROWS 256          /* rows per workgroup of gf_ppo_loss: one partial record per workgroup */
#define GF_PPO_OUT_COUNT 5             /* out[]: surrogate, value_loss, entropy, kl_mean, loss */
/* workspace of gf_ppo_loss: (3 + A) doubles per workgroup of rows, 8-byte aligned */
#define GF_PPO_LOSS_WORKSPACE_BYTES(mb, A) ((int64_t)(((mb) + GF_PPO_BLOCK_ROWS - 1) / GF_PPO_BLOCK_ROWS) * (3 + (int64_t)(A)) * 8)
#define GF_ADAM_BLOCK_ELEMS 1024       /* elements per workgroup and pass of gf_adam_step (256 lanes x 4) */
#define GF_ADAM_MAX_PARTIALS 1024      /* norm partials (workgroups of launch 1) at most */
/* workspace of gf_adam_step: one double per launch-1 workgroup, 8-byte aligned */
#define GF_ADAM_WORKSPACE_BYTES(numel) \
    ((int64_t)((((numel) + GF_ADAM_BLOCK_ELEMS - 1) / GF_ADAM_BLOCK_ELEMS) < GF_ADAM_MAX_PARTIALS ? \
               (((numel) + GF_ADAM_BLOCK_ELEMS - 1) / GF_ADAM_BLOCK_ELEMS) : GF_ADAM_MAX_PARTIALS) * 8)
#define GF_ADAM_SCHEDULE_FIXED 0
#define GF_ADAM_SCHEDULE_ADAPTIVE 1

typedef struct GfPpoLossArgs {
    int64_t num_rows;           /* mb >= 0; 0: nothing is launched */
    int32_t num_actions;        /* A >= 1 */
    int32_t use_clipped_value_loss;   /* 0 or 1 */
    const float* mu;            /* [mb, A] actor mean of this update */
    const float* sigma;         /* [A] action std (shared by every row), or log_std with sigma_is_log */
    const float* value;         /* [mb] critic output of this update */
    const float* actions;       /* [mb, A] minibatch actions */
    const float* old_log_prob;  /* [mb] */
    const float* advantages;    /* [mb] */
    const float* target_values; /* [mb] values stored with the rollout */
    const float* returns;       /* [mb] */
    const float* old_mu;        /* [mb, A] */
    const float* old_sigma;     /* [mb, A] */
    float clip_param;
    float value_loss_coef;
    float entropy_coef;
    int32_t sigma_is_log;       /* 0: `sigma` is the std, 1: it is log_std and grad_sigma receives d loss / d log_std */
    float* grad_mu;             /* [mb, A] d loss / d mu, or NULL: no gradients (then all three are NULL) */
    float* grad_value;          /* [mb] */
    float* grad_sigma;          /* [A] d loss / d sigma (d loss / d log_std with sigma_is_log) */
    float* out;                 /* [GF_PPO_OUT_COUNT] (required) */
    double* sums;               /* [3] += value_loss, surrogate, entropy (rsl_rl's loss-dict order), or NULL */
    void* workspace;            /* GF_PPO_LOSS_WORKSPACE_BYTES(mb, A) bytes, 8-byte aligned */
    int64_t workspace_bytes;
    int64_t kl_rows;            /* 0: the KL covers all mb rows; 1 … mb: the first kl_rows rows only (old_mu / old_sigma are then [kl_rows, A]) */
} GfPpoLossArgs;

typedef struct GfAdamState {    /* device control block; GfAdamArgs.state points at two of them */
    double lr;                  /* learning rate (double, as Python keeps it) */
    int64_t step;               /* Adam steps taken */
} GfAdamState;

typedef struct GfAdamArgs {
    int64_t numel;              /* >= 0; 0: nothing is launched */
    float* params;              /* [numel] flat parameters, updated in place */
    float* grads;               /* [numel] flat gradient; the clipped gradient is written back */
    float* exp_avg;             /* [numel] */
    float* exp_avg_sq;          /* [numel] */
    GfAdamState* state;         /* [2]: slot `parity` is read, slot 1 - parity written */
    const float* kl_mean;       /* the KL of the adaptive schedule (required with it, NULL with the fixed one) */
    void* workspace;            /* GF_ADAM_WORKSPACE_BYTES(numel) bytes, 8-byte aligned */
    int64_t workspace_bytes;
    double desired_kl;          /* > 0 with the adaptive schedule */
    double beta1, beta2, eps;   /* as Python holds them (torch defaults 0.9, 0.999, 1e-8): b^step in double, the rest rounded to f32 */
    float max_grad_norm;        /* > 0 */
    int32_t schedule;           /* GF_ADAM_SCHEDULE_FIXED / _ADAPTIVE */
    int32_t parity;             /* 0 or 1 */
    int32_t _pad;
} GfAdamArgs;

/* ------------------------------------------------------------------------------------------
 * Mirror symmetry of the PPO update (rsl_rl's symmetry_cfg: data augmentation and mirror loss for a left/right symmetric robot).
 * A mirror is a signed permutation per tensor kind:  mirror(x)[n, j] = sign[j] · x[n, perm[j]].  rsl_rl runs a Python callback, a
 * torch.cat per field, a repeat per scalar and an MSELoss with its backward per minibatch; here:
 *
 * gf_mirror_rows — ONE launch for up to GF_MIRROR_MAX_FIELDS row fields (observations, critic observations, actions, one spare) and
 * up to GF_MIRROR_MAX_SCALARS per-row scalars (old log-prob, advantages, target values, returns).  Per field
 *     dst_copy  [n, j] = f_j(src[n, j])                       (dst_copy == NULL: not written)
 *     dst_mirror[n, j] = f_j(sign[j] · src[n, perm[j]])
 * with f_j the identity, or with a normaliser (in_mean != NULL)  f_j(v) = (v - in_mean[j]) / (in_std[j] + in_eps)  — one
 * subtraction, one addition, one correctly rounded division, the operations of gf_minibatch_gather and gf_mlp_act.  The mirror is
 * taken of the RAW value and normalised at the DESTINATION column: rsl_rl augments first and normalises inside the policy.  Source
 * row n is at src + n · row_stride (0: width, as GfMlpSegment); the two destinations have contiguous rows and usually are the two
 * halves of one [2·rows, width] tensor.  Per scalar  dst[i] = dst[rows + i] = src[i].
 * A workgroup stages a tile of source rows in LDS — every source row is read from memory once — and writes both destinations from it;
 * 16-byte loads and stores where the width, the row stride and every pointer of the field allow it, by element otherwise.  No atomics,
 * no workspace, no allocation, no synchronisation.  Bit-exact: a signed permutation rounds nothing.
 * `perm` / `sign` are TRUSTED: the entry point cannot look at device memory, an entry outside 0 … width-1 reads outside the tile.
 * They come from genesis_forge_amd.MirrorSymmetry, which validates on the host (a permutation, signs ±1, an involution) before it
 * uploads them; no caller may hand over anything else.
 * Refusals, before anything is launched: GF_E_NULL — args, a field's src / dst_mirror / perm / sign, in_mean without in_std, a
 * scalar's src / dst; GF_E_RANGE — num_rows < 0, num_fields outside 0 … GF_MIRROR_MAX_FIELDS, num_scalars outside 0 …
 * GF_MIRROR_MAX_SCALARS, both zero, a width outside 1 … GF_MIRROR_MAX_WIDTH, a non-zero row_stride < width.  num_rows == 0 is a no-op.
 *
 * gf_mirror_loss — rsl_rl's symmetry loss  MSE(actor(mirror(obs)), mirror(actor(obs)).detach())  and its gradient:
 *     d[n, j] = mu_mirror[n, j] - sign[j] · mu_orig[n, perm[j]]            (one rounding)
 *     loss    = mean over the mb·A elements of d²   -> out[0] (float32), and sums[0] += (double)out[0] when sums != NULL
 *     grad[n, j] += coeff · 2 · d[n, j] / (mb·A)                           (grad != NULL; mu_orig is a constant: no gradient)
 * as ((coeff · inv) · (2 · d)) with inv = 1 / (float)(mb·A): three more roundings, then the addition into what `grad` holds — the
 * mirrored half of gf_ppo_loss's grad_mu when augmenting, a zeroed buffer otherwise.  grad == NULL is the logging-only mode: nothing
 * but out / sums is written.  The shape of gf_ppo_loss: one lane per row, one double partial per workgroup in the caller's
 * workspace, a second one-workgroup launch sums them in a fixed order.  No atomics: bitwise reproducible.  `perm` / `sign` are the
 * action tables, trusted as above.
 * Refusals: GF_E_NULL — args, mu_mirror, mu_orig, perm, sign, out, workspace; GF_E_RANGE — num_rows < 0, num_actions < 1, a
 * workspace smaller than GF_MIRROR_LOSS_WORKSPACE_BYTES(mb) or not 8-byte aligned.  num_rows == 0 is a no-op.
 * Neither is a phase of the step.
 * ---------------------------------------------------------------------------------------- */
#define GF_MIRROR_MAX_FIELDS 4
#define GF_MIRROR_MAX_SCALARS 4
#define GF_MIRROR_MAX_WIDTH 8192       /* floats of the LDS tile: one row must fit */
#define GF_MIRROR_LOSS_BLOCK_ROWS 256  /* rows per workgroup of gf_mirror_loss: one double partial per workgroup */
#define GF_MIRROR_LOSS_WORKSPACE_BYTES(mb) ((int64_t)(((mb) + GF_MIRROR_LOSS_BLOCK_ROWS - 1) / GF_MIRROR_LOSS_BLOCK_ROWS) * 8)

typedef struct GfMirrorField {
    const float* src;           /* [rows, width], row n at src + n * row_stride */
    float* dst_copy;            /* [rows, width] contiguous, or NULL */
    float* dst_mirror;          /* [rows, width] contiguous */
    const int32_t* perm;        /* [width] source column of destination column j (trusted: 0 … width-1) */
    const float* sign;          /* [width] ±1 */
    const float* in_mean;       /* [width] normaliser mean, or NULL: f_j is the identity */
    const float* in_std;        /* [width] normaliser std (required with in_mean) */
    float in_eps;               /* added to in_std */
    int32_t width;              /* 1 … GF_MIRROR_MAX_WIDTH */
    int32_t row_stride;         /* floats from a source row to the next; 0: `width`; otherwise >= width */
    int32_t _pad;
} GfMirrorField;

typedef struct GfMirrorScalar {
    const float* src;           /* [rows] */
    float* dst;                 /* [2 * rows]: both halves receive src */
} GfMirrorScalar;

typedef struct GfMirrorRowsArgs {
    int64_t num_rows;           /* rows >= 0; 0: nothing is launched */
    int32_t num_fields;         /* 0 … GF_MIRROR_MAX_FIELDS */
    int32_t num_scalars;        /* 0 … GF_MIRROR_MAX_SCALARS (not both 0) */
    GfMirrorField fields[GF_MIRROR_MAX_FIELDS];
    GfMirrorScalar scalars[GF_MIRROR_MAX_SCALARS];
} GfMirrorRowsArgs;

typedef struct GfMirrorLossArgs {
    int64_t num_rows;           /* mb >= 0; 0: nothing is launched */
    int32_t num_actions;        /* A >= 1 */
    float coeff;                /* mirror_loss_coeff: scales the gradient only (the loss is logged unscaled) */
    const float* mu_mirror;     /* [mb, A] the actor on the mirrored observations */
    const float* mu_orig;       /* [mb, A] the actor on the originals (a constant) */
    const int32_t* perm;        /* [A] action tables (trusted) */
    const float* sign;          /* [A] */
    float* grad;                /* [mb, A] += coeff · d loss / d mu_mirror, or NULL: loss only */
    float* out;                 /* [1] the loss (required) */
    double* sums;               /* [1] += the loss, or NULL */
    void* workspace;            /* GF_MIRROR_LOSS_WORKSPACE_BYTES(mb) bytes, 8-byte aligned */
    int64_t workspace_bytes;
} GfMirrorLossArgs;

/* ------------------------------------------------------------------------------------------
 * The actor-critic forward of a collection step (rsl_rl ActorCritic.act / evaluate inside PPO.act): torch runs each MLP as one GEMM
 * and one ELU launch per layer — 14 launches for the obs -> 512 -> 256 -> 128 -> A / 1 nets of the reference configs — and every
 * activation makes a round trip through memory.  gf_mlp_act runs both nets AND the whole of gf_policy_act in ONE launch:
 *     observations        -> actor MLP  -> mean  -> sample, log_prob, the policy's storage rows (gf_policy_act's contract, word for word)
 *     critic observations -> critic MLP -> value -> storage row
 * A workgroup owns GF_MLP_TILE_ROWS rows of ONE net (grid y: actor / critic; the two have no data dependency), walks its layers on
 * the f32 matrix cores (v_mfma_f32_32x32x2_f32) and keeps the tile's activations in LDS; only mean, values, actions and the storage
 * rows are written to memory.  Weights are read in place, `[out, in]` row-major f32 exactly as torch.nn.Linear stores them; the first
 * layer reads its input as up to GF_MLP_MAX_INPUTS segments `[N, width]` side by side (an observation group of several managers
 * needs no torch.cat); a segment's rows are `row_stride` floats apart (0: `width`, contiguous rows) — the strided view an
 * ObservationManager with output="window" hands out is read in place.  Layers are Linear with ELU(alpha = 1) between them and none after the last.
 *
 * Arithmetic (the one exception to "a left fold of separately rounded operations"):
 *     y[n, j] = chain over k = 0 … K-1, ascending, of fma(x[n, k], W[j, k], acc),  acc starting from bias[j];
 *     hidden layers then  v > 0 ? v : expm1f(v).
 * One chain per output element, no split-K, no atomics: row n's results depend on row n's inputs only — not on num_envs, the tile it
 * falls in, env_offset or the run.  The f32 MFMA is bit for bit such a chain (one rounding per fma, f32 accumulator).
 *
 * Input normalisation (rsl_rl EmpiricalNormalization.forward in front of a net; `in_mean == NULL`: none, the path above bit for bit):
 *     x[n, k] = (obs[n, k] - in_mean[k]) / (in_std[k] + in_eps)     (one subtraction, one addition, one correctly rounded division)
 * applied to every real element as the first layer's input is staged — k is the column of the whole input, across the segments; the
 * zero padding of rows past num_envs and of columns past the input width stays zero.  No launch and no [N, W] tensor of its own.
 *
 * Either net may be absent (num_layers == 0): actor only = play-time inference, critic only = the bootstrap value.  With an actor,
 * `actions == NULL` computes the mean only and draws nothing (then `mean` is required and actions_out / mu_out / sigma_out /
 * log_prob_out must be NULL).  `mean` / `values` are optional fresh outputs.  std_is_log = 1: `std` holds log_std, as
 * GfPolicyActArgs.std_is_log (the flag is forwarded to the same row code; without `actions` it is only range-checked).
 * Refusals, before anything is launched: GF_E_NULL — args, a weight / bias / segment pointer, in_mean without in_std, std with
 * actions, an actor without mean and actions, a critic without values and values_out, an actor's or critic's output pointer with that net absent;
 * GF_E_RANGE — num_envs < 0, more than GF_MLP_MAX_LAYERS layers, a segment count outside 1 … GF_MLP_MAX_INPUTS, a width < 1, a
 * non-zero row_stride < width, a hidden width > GF_MLP_MAX_HIDDEN, a total input width > GF_MLP_MAX_INPUT_WIDTH, an actor output > GF_MLP_MAX_ACTIONS,
 * std_per_env or std_is_log outside {0, 1}; GF_E_UNSUPPORTED — both nets absent, a critic output other than 1.  num_envs == 0 is a no-op.
 * No allocation, no copy, no synchronisation inside.  Not a phase of the step.
 * ---------------------------------------------------------------------------------------- */
#define GF_MLP_MAX_LAYERS 6            /* Linear layers per net */
#define GF_MLP_MAX_INPUTS 4            /* input segments per net */
#define GF_MLP_MAX_HIDDEN 512          /* widest hidden layer */
#define GF_MLP_MAX_INPUT_WIDTH 1024    /* sum of the segment widths */
#define GF_MLP_MAX_ACTIONS 64          /* widest actor output */
#define GF_MLP_TILE_ROWS 32            /* rows per workgroup */

typedef struct GfMlpSegment {
    const float* rows;          /* [N, width], row n at rows + n * row_stride */
    int32_t width;              /* >= 1 */
    int32_t row_stride;         /* floats from a row to the next; 0: `width` (contiguous rows); otherwise >= width */
} GfMlpSegment;

typedef struct GfMlpLayer {
    const float* weight;        /* [out_width, in] row-major, torch.nn.Linear.weight read in place */
    const float* bias;          /* [out_width] */
    int32_t out_width;          /* >= 1; `in` is the previous layer's out_width (layer 0: the sum of the segment widths) */
    int32_t _pad;
} GfMlpLayer;

typedef struct GfMlpNet {
    int32_t num_layers;         /* 1 … GF_MLP_MAX_LAYERS; 0: the net is absent */
    int32_t num_inputs;         /* 1 … GF_MLP_MAX_INPUTS */
    GfMlpSegment inputs[GF_MLP_MAX_INPUTS];
    GfMlpLayer layers[GF_MLP_MAX_LAYERS];
    const float* in_mean;       /* [input width] normaliser mean spanning all segments, or NULL: the input is read as it is */
    const float* in_std;        /* [input width] normaliser std (required with in_mean) */
    float in_eps;               /* added to in_std */
    int32_t _pad;
} GfMlpNet;

typedef struct GfMlpActArgs {
    int64_t num_envs;           /* N >= 0; 0: nothing is launched */
    GfMlpNet actor;             /* output width A <= GF_MLP_MAX_ACTIONS */
    GfMlpNet critic;            /* output width 1 */
    const float* std;           /* [A] or [N, A] (required with actions): the std, or log_std with std_is_log */
    const float* noise;         /* [N, A] standard normals (parity mode), or NULL: Philox + Box–Muller */
    uint64_t seed;              /* as GfPolicyActArgs */
    uint64_t stream;
    uint32_t env_offset;
    int32_t std_per_env;        /* 0: std is [A], 1: [N, A] */
    float* mean;                /* [N, A] out: the actor's output, or NULL */
    float* values;              /* [N] out: the critic's output, or NULL */
    float* actions;             /* [N, A] out: the sample, or NULL: mean only */
    float* actions_out;         /* storage rows, as GfPolicyActArgs; each may be NULL */
    float* mu_out;
    float* sigma_out;
    float* values_out;
    float* log_prob_out;
    int32_t std_is_log;         /* 0: `std` is the std, 1: it is log_std (sigma = expf), as GfPolicyActArgs */
    int32_t _pad;
} GfMlpActArgs;

/* ------------------------------------------------------------------------------------------
 * The collection step of a recurrent policy (rsl_rl ActorCriticRecurrent.act / evaluate inside PPO.act: a one-layer LSTM or GRU
 * `Memory` in front of the actor MLP and another in front of the critic MLP).  In torch that is gf_mlp_act's 14 launches, two RNN
 * calls on a sequence of length one and the hidden-state bookkeeping (the masked reset on `dones`, the copy of the state into the
 * storage).  gf_mlp_recurrent_act is gf_mlp_act's launch with a cell between the input and the MLP of a net:
 *     observations -> normaliser -> cell (h, c read; h', c' stored in place) -> h' -> MLP -> gf_mlp_act's outputs, word for word
 * `act` is a gf_mlp_act descriptor; a net's segments (and in_mean / in_std) describe the CELL's input, of width `in` = the sum of the
 * segment widths, and its layers[0] reads `hidden` columns.  A net whose cell has type GF_RNN_NONE is gf_mlp_act's net unchanged.
 *
 * The cell (torch.nn.LSTM / torch.nn.GRU with one layer, their tensors read in place; G = 4 gates i, f, g, o for LSTM, G = 3 gates
 * r, z, n for GRU, gate g of unit j being row g · H + j):
 *     h0, c0 = reset[n] != 0 ? 0 : h[n], c[n]                               (h_save / c_save, when given, receive h0 / c0)
 *     LSTM:  p_g[j] = chain from (b_ih[gH + j] + b_hh[gH + j])  — one f32 addition — over k = 0 … in-1 of fma(x[n, k], w_ih[gH + j, k], ·),
 *                     ascending, then over k = 0 … H-1 of fma(h0[k], w_hh[gH + j, k], ·), ascending: ONE chain per gate element;
 *            c' = fl(fl(sig(p_f) · c0) + fl(sig(p_i) · tanh(p_g))),   h' = fl(sig(p_o) · tanh(c'))
 *     GRU:   p_r, p_z as above;  n_x[j] = chain from b_ih[2H + j] over the input columns,  n_h[j] = chain from b_hh[2H + j] over the
 *            hidden columns (two chains: r multiplies the second only);
 *            n = tanh(fl(n_x + fl(sig(p_r) · n_h))),   h' = fl(fl(fl(1 - sig(p_z)) · n) + fl(sig(p_z) · h0))
 *     sig(p) = 1.0f / (1.0f + expf(-p)) — one negation, the device libm's expf, one addition, one correctly rounded division;
 *     tanh is the device libm's tanhf.  Every fl() is one f32 rounding (no contraction).
 * h[n] and c[n] are then overwritten with h' and c' ([N, H], torch's [1, N, H] state viewed flat): a workgroup touches its own rows
 * only, so in place is safe.  The MLP's first Linear reads h' as its input and the walk goes on as in gf_mlp_act: with the same h'
 * handed to gf_mlp_act as a one-segment observation of width H and the same layers, mean, values, actions and every storage row are
 * bit for bit gf_mlp_act's.  Row n's results depend on row n's inputs only — not on num_envs, the tile, or the other net.
 *
 * LDS: the tile's x pass and its h0 side by side, 2 × 65 664 B: one workgroup per CU (gf_mlp_act has two).  A wave keeps the four
 * gate columns of one 32-unit block in its four accumulators; H > 128 takes (H / 32 + 3) / 4 rounds over the same staged x and h0.
 *
 * Refusals, before anything is launched: everything gf_mlp_act refuses for `act`, with its codes; GF_E_RANGE — a cell type outside
 * GF_RNN_NONE … GF_RNN_GRU, `hidden` outside 1 … GF_MLP_MAX_HIDDEN, a cell on an absent net; GF_E_NULL — w_ih, w_hh, b_ih, b_hh or h
 * missing, an LSTM without c, a GRU with c or c_save, h_save or c_save with GF_RNN_NONE; GF_E_UNSUPPORTED — both cells GF_RNN_NONE
 * (gf_mlp_act is the call for that).  num_envs == 0 is a no-op.  No allocation, no copy, no synchronisation inside.
 * ---------------------------------------------------------------------------------------- */
#define GF_RNN_NONE 0
#define GF_RNN_LSTM 1
#define GF_RNN_GRU 2

typedef struct GfRnnCell {
    int32_t type;               /* GF_RNN_NONE: the net has no cell; GF_RNN_LSTM; GF_RNN_GRU */
    int32_t hidden;             /* H, 1 … GF_MLP_MAX_HIDDEN */
    const float* w_ih;          /* [G * H, in] row-major: weight_ih_l0 read in place */
    const float* w_hh;          /* [G * H, H]: weight_hh_l0 */
    const float* b_ih;          /* [G * H] */
    const float* b_hh;          /* [G * H] */
    float* h;                   /* [N, H] in/out: the hidden state */
    float* c;                   /* [N, H] in/out: the cell state (LSTM); NULL for GRU */
    const uint8_t* reset;       /* [N] or NULL: a row with reset[n] != 0 reads zeros for h[n] / c[n] */
    float* h_save;              /* [N, H] or NULL: out, the state the step started from (after the reset) */
    float* c_save;              /* [N, H] or NULL (LSTM only) */
} GfRnnCell;

typedef struct GfMlpRecurrentActArgs {
    GfMlpActArgs act;           /* gf_mlp_act's descriptor: a net with a cell reads `hidden` columns in layers[0] */
    GfRnnCell actor_cell;
    GfRnnCell critic_cell;
} GfMlpRecurrentActArgs;

/* ------------------------------------------------------------------------------------------
 * The trajectory minibatches of a recurrent policy's update (rsl_rl split_and_pad_trajectories and
 * RolloutStorage.recurrent_mini_batch_generator).  A rollout `[T, N]` is cut into trajectories at the dones — dones[T-1] counts as
 * set — and enumerated env-major: env 0's in time order, then env 1's, …  A minibatch is a contiguous env range, so its
 * trajectories are a contiguous range of that enumeration.
 *
 * gf_traj_table, once per update: counts[n] = the trajectories of env n, offsets[n] = their exclusive prefix sum (offsets[N] = the
 * total), table[j] = (env, t0, len) of trajectory j, `[T · N, 3]` int32 of which the first offsets[N] rows are written.  One
 * workgroup scans the envs 256 at a time (wave shuffle scan, wave totals through LDS, a carried total): deterministic, no atomics.
 * Refusals: GF_E_NULL — args or a pointer; GF_E_RANGE — a negative size, T · N > (2^31 - 1) / 3.  T == 0 or N == 0 is a no-op.
 *
 * gf_traj_gather, one launch per minibatch = the trajectories [first_traj, first_traj + num_traj) of the envs
 * [env_start, env_start + num_mb_envs):
 *     groups[g].dst `[T, num_traj, W]`   row (s, j) = the group's observation of step t0_j + s of env_j for s < len_j — its segments side
 *                                        by side (row (t, n) of a segment at rows + (t · N + n) · row_stride; 0: width), through the
 *                                        normaliser where `mean` is given: (v - mean[k]) / (std[k] + eps), gf_minibatch_gather's
 *                                        operations — and zeros from len_j on (padding is not normalised).  width == 0: no such group.
 *     masks `[T, num_traj]` uint8        1 where s < len_j
 *     unpad_index `[num_mb_envs · T]`    element (env - env_start) · T + t = j · T + (t - t0_j): where step t of that env sits in the
 *                                        `[num_traj, T]`-flattened padded batch (index_select on it is rsl_rl's unpad_trajectories)
 *     states[k].h0 / c0 `[num_traj, H]`  the rollout-start state h_start / c_start `[N, H]` of env_j where t0_j == 0, zeros elsewhere:
 *                                        a trajectory that starts later starts behind a done.  hidden == 0: no such net; c0 NULL: a GRU.
 * Refusals: GF_E_NULL — args, table, masks, unpad_index, a group's dst / segment, mean without std, h_start / h0, c0 without
 * c_start, a pointer of an absent group or net; GF_E_RANGE — sizes < 1 (num_traj, first_traj, env_start, num_mb_envs < 0), an env
 * range past num_envs, num_traj outside num_mb_envs … T · num_mb_envs, a trajectory range past table_rows, a segment count outside
 * 1 … GF_MLP_MAX_INPUTS, segment widths that do not add up to `width`, width > GF_MLP_MAX_INPUT_WIDTH, hidden > GF_MLP_MAX_HIDDEN.
 * num_traj == 0 is a no-op.  No allocation, no copy, no synchronisation inside either.
 * ---------------------------------------------------------------------------------------- */
typedef struct GfTrajTableArgs {
    int32_t num_steps;          /* T */
    int32_t num_envs;           /* N */
    const uint8_t* dones;       /* [T, N] */
    int32_t* counts;            /* [N] out */
    int32_t* offsets;           /* [N + 1] out */
    int32_t* table;             /* [T * N, 3] out: (env, t0, len) */
} GfTrajTableArgs;

typedef struct GfTrajGroup {
    int32_t num_inputs;         /* 1 … GF_MLP_MAX_INPUTS */
    int32_t width;              /* W = the sum of the segment widths; 0: the group is absent */
    GfMlpSegment inputs[GF_MLP_MAX_INPUTS];   /* [T * N, width] each */
    const float* mean;          /* [W] or NULL */
    const float* std;           /* [W] (required with mean) */
    float eps;
    int32_t _pad;
    float* dst;                 /* [T, num_traj, W] out */
} GfTrajGroup;

typedef struct GfTrajState {
    int32_t hidden;             /* H; 0: the net is absent */
    int32_t _pad;
    const float* h_start;       /* [N, H] the rollout-start state */
    const float* c_start;       /* [N, H] (with c0) */
    float* h0;                  /* [num_traj, H] out */
    float* c0;                  /* [num_traj, H] out, or NULL */
} GfTrajState;

typedef struct GfTrajGatherArgs {
    int32_t num_steps;          /* T */
    int32_t num_envs;           /* N */
    int32_t first_traj;
    int32_t num_traj;
    int32_t env_start;
    int32_t num_mb_envs;
    int32_t table_rows;         /* rows of `table` that gf_traj_table wrote (offsets[N]) */
    int32_t _pad;
    const int32_t* table;       /* gf_traj_table's */
    GfTrajGroup groups[2];      /* the actor's and the critic's observation group */
    GfTrajState states[2];      /* the actor's and the critic's memory */
    uint8_t* masks;             /* [T, num_traj] out */
    int64_t* unpad_index;       /* [num_mb_envs * T] out */
} GfTrajGatherArgs;

/* ------------------------------------------------------------------------------------------
 * The collection step of teacher–student distillation (rsl_rl Distillation.act: StudentTeacher.act on the deployable observations,
 * StudentTeacher.evaluate on the privileged ones).  The two MLPs have no data dependency, and at a few thousand envs one net leaves
 * half the device idle (N / GF_MLP_TILE_ROWS workgroups per net): gf_mlp_distill_act runs both in ONE launch, grid y = net, with
 * gf_mlp_act's tile, LDS and weight-streaming scheme and its layer code unchanged:
 *     observations            -> student MLP -> mean -> sample (gf_policy_act's row code) -> actions, actions_out
 *     privileged observations -> teacher MLP -> teacher_actions, teacher_actions_out
 * Each net is a GfMlpNet of its own — segments, row_stride, layers, optional in_mean / in_std / in_eps — so depth, input width and
 * normaliser may differ; both outputs are A <= GF_MLP_MAX_ACTIONS wide.  Nothing of the teacher is sampled; no value, log-probability,
 * mu or sigma row is written.
 *
 * Arithmetic: a row's results are the k-ascending fma chains of gf_mlp_act (see above), so
 *     actions, mean, actions_out  ==  those of a gf_mlp_act launch with `student` as its actor and the same std / std_is_log, noise,
 *                                     seed, stream and env_offset, bit for bit;
 *     teacher_actions (and teacher_actions_out)  ==  the `mean` of a gf_mlp_act launch with `teacher` as its actor, bit for bit.
 * `std` is [A] (std_is_log = 1: log_std, as GfPolicyActArgs.std_is_log).
 * Refusals, before anything is launched: GF_E_NULL — args, a weight / bias / segment pointer, in_mean without in_std, std, actions,
 * teacher_actions; GF_E_RANGE — num_envs < 0, std_is_log outside {0, 1}, what gf_mlp_act ranges per net (layer and segment counts,
 * widths, row_stride, hidden and input widths, an output > GF_MLP_MAX_ACTIONS), student and teacher output widths that differ;
 * GF_E_UNSUPPORTED — either net absent (num_layers == 0).  num_envs == 0 is a no-op.
 * No allocation, no copy, no synchronisation inside.  Not a phase of the step.
 * ---------------------------------------------------------------------------------------- */
typedef struct GfMlpDistillArgs {
    int64_t num_envs;           /* N >= 0; 0: nothing is launched */
    GfMlpNet student;           /* output width A <= GF_MLP_MAX_ACTIONS */
    GfMlpNet teacher;           /* output width A */
    const float* std;           /* [A] (required): the student's std, or log_std with std_is_log */
    const float* noise;         /* [N, A] standard normals (parity mode), or NULL: Philox + Box–Muller */
    uint64_t seed;              /* as GfPolicyActArgs */
    uint64_t stream;
    uint32_t env_offset;
    int32_t std_is_log;         /* 0: `std` is the std, 1: it is log_std (sigma = expf) */
    float* mean;                /* [N, A] out: the student's output, or NULL */
    float* actions;             /* [N, A] out: the sample (required) */
    float* actions_out;         /* [N, A] the storage row of the sample, or NULL */
    float* teacher_actions;     /* [N, A] out: the teacher's output (required) */
    float* teacher_actions_out; /* [N, A] a second destination of it (the storage row), or NULL */
} GfMlpDistillArgs;

/* ------------------------------------------------------------------------------------------
 * The collection step of distillation with a recurrent student (rsl_rl Distillation.act on a StudentTeacherRecurrent: memory_s in
 * front of the student MLP, optionally memory_t in front of the teacher MLP).  gf_mlp_recurrent_distill_act is gf_mlp_distill_act's
 * launch — grid (tiles of GF_MLP_TILE_ROWS rows, 2), y = 0 the student, y = 1 the teacher — with gf_mlp_recurrent_act's walk per
 * workgroup: normaliser -> cell (state read, reset where flagged, advanced and stored in place, h_save / c_save written) -> MLP ->
 * gf_mlp_distill_act's finish (the student: mean, sampling, actions_out; the teacher: its output to both destinations).  The cell's
 * arithmetic and gate layout are those documented above GfRnnCell, the LDS and occupancy those of gf_mlp_recurrent_act.  A net whose
 * cell is GF_RNN_NONE is gf_mlp_distill_act's net unchanged.
 *
 * Bit for bit: the student's actions, mean, actions_out, h, c, h_save, c_save equal those of a gf_mlp_recurrent_act launch with
 * `student` as the actor, student_cell as actor_cell, no critic and the same std / std_is_log / noise / seed / stream / env_offset
 * (gf_mlp_act where student_cell is GF_RNN_NONE); teacher_actions, teacher_actions_out and the teacher's state equal the `mean` and
 * state of such a launch with `teacher` as the actor.  Row n depends on row n only; rows past num_envs are never written.
 *
 * Refusals, before anything is launched: everything gf_mlp_distill_act refuses for `act` and everything gf_mlp_recurrent_act refuses
 * per cell, with their codes; GF_E_UNSUPPORTED — both cells GF_RNN_NONE (gf_mlp_distill_act is the call for that).  num_envs == 0 is
 * a no-op.  No allocation, no copy, no synchronisation inside.  Not a phase of the step.
 * ---------------------------------------------------------------------------------------- */
typedef struct GfMlpRecurrentDistillArgs {
    GfMlpDistillArgs act;       /* gf_mlp_distill_act's descriptor; a net with a cell: its segments / in_mean / in_std describe the CELL's
                                   input, its layers[0] reads `hidden` columns (as GfMlpRecurrentActArgs) */
    GfRnnCell student_cell;
    GfRnnCell teacher_cell;     /* GF_RNN_NONE: that net is gf_mlp_distill_act's net unchanged */
} GfMlpRecurrentDistillArgs;

/* ------------------------------------------------------------------------------------------
 * The curiosity bonus of a collection step (rsl_rl RandomNetworkDistillation.get_intrinsic_reward and the `rewards += intrinsic` of
 * PPO.process_env_step): a frozen random `target` MLP and a trained `predictor` MLP read the same rnd_state rows, the distance of
 * their outputs is the intrinsic reward.  rsl_rl spends about twenty small launches and one host read (`if std > 0`) on it;
 * gf_rnd_reward is ONE launch without the reward normaliser (or with it in eval mode) and TWO with it updating, no host read.
 *     x       = (rnd_state - in_mean) / (in_std + in_eps)             (the state normaliser: each net's in_mean / in_std / in_eps)
 *     t, p    = target(x), predictor(x)                               (gf_mlp_act's k-ascending fma chains: a row's embedding is the
 *                                                                      `mean` of a gf_mlp_act launch with that net as actor, bit for bit)
 *     r[n]    = (float)sqrt(Σ_j (double)(t[n,j] - p[n,j])²)           (d_j one f32 subtraction; j ascending; the sum in double)
 * normalize == 0:  i = r · weight.
 * normalize == 1 (rsl_rl EmpiricalDiscountedVariationNormalization), update == 1 (training mode):
 *     avg[n]  = first ? r[n] : avg[n]·gamma + r[n]                    (one f32 multiply, one f32 add, not contracted)
 *     unless until >= 0 and count >= until: mean / var / std / count take EmpiricalNormalization.update's lines on the N values of
 *     avg as one batch (gf_obs_norm_update's arithmetic: batch moments and the update in float64, rounded to f32 once; std = sqrtf(var))
 *   then, and with update == 0 at once (avg and the statistics are not touched):
 *     i = (std > 0 ? r / std : r) · weight                            (the std after the update; no eps in this division)
 * Either way:  intrinsic[n] = i;  with rewards != NULL:  acc_extrinsic[n] += rewards[n] (where given), rewards[n] = rewards[n] + i;
 * acc_intrinsic[n] += i (where given).  The accumulators are per env: the caller's means need no reduction in the kernel.
 *
 * Launch 1 is gf_mlp_act's tile (GF_MLP_TILE_ROWS rows per workgroup, weights streamed, activations in LDS): the workgroup walks the
 * target, keeps the tile's E outputs in a second LDS array, walks the predictor from the re-staged input; lane r finishes row r.
 * With the normaliser updating it stores r in `intrinsic`, the new avg, one {rows, mean, M2} record of the tile's avg per workgroup
 * and — workgroup 0 — the old mean / var / std / count in the workspace header.  Launch 2 (256 rows per workgroup): every workgroup
 * folds the records in the same fixed order (gf_reduce.h) and applies the update from the header's snapshot, so all hold the same
 * new std; workgroup 0 alone stores the statistics, nobody reads the live ones.  No atomics: bitwise reproducible.
 * Refusals, before anything is launched: GF_E_NULL — args, a weight / bias / segment pointer, in_mean without in_std, intrinsic,
 * workspace, avg / mean / var / std / count with normalize; GF_E_RANGE — num_envs < 0, normalize / update / first outside {0, 1},
 * what gf_mlp_act ranges per net, output widths that differ, segment sets that differ (count, rows, width, row_stride), a workspace
 * smaller than GF_RND_WORKSPACE_BYTES(N) or not 8-byte aligned, a count pointer not 8-byte aligned; GF_E_UNSUPPORTED — either net
 * absent.  num_envs == 0 is a no-op.  No allocation, no copy, no synchronisation inside.  Not a phase of the step.
 * ---------------------------------------------------------------------------------------- */
/* header of four doubles (the old mean, var, std, count) + {rows, mean, M2} per tile of GF_MLP_TILE_ROWS rows */
#define GF_RND_WORKSPACE_BYTES(n) ((int64_t)(4 + 3 * (((int64_t)(n) + GF_MLP_TILE_ROWS - 1) / GF_MLP_TILE_ROWS)) * 8)

typedef struct GfRndRewardArgs {
    int64_t num_envs;           /* N >= 0; 0: nothing is launched */
    GfMlpNet target;            /* the frozen net; output width E <= GF_MLP_MAX_ACTIONS */
    GfMlpNet predictor;         /* the trained net: the same segments, output width E */
    float weight;               /* the schedule's current weight (computed on the host, passed by value) */
    float gamma;                /* the reward normaliser's own discount */
    int32_t normalize;          /* 1: the reward normaliser divides by its std */
    int32_t update;             /* 1 (with normalize): avg and the statistics are updated first (training mode) */
    int32_t first;              /* 1 (with update): the first call — avg = r */
    int32_t _pad;
    float* avg;                 /* [N] per-env discounted sum, in and out (required with normalize) */
    float* mean;                /* [1] running statistics of avg (required with normalize) */
    float* var;                 /* [1] */
    float* std;                 /* [1] */
    int64_t* count;             /* one word (required with normalize) */
    int64_t until;              /* >= 0: no update of the statistics once count >= until; negative: none */
    float* rewards;             /* [N] the storage row, added to in place, or NULL */
    float* intrinsic;           /* [N] out: the weighted intrinsic reward (required) */
    double* acc_extrinsic;      /* [N] += rewards[n] before the add, or NULL */
    double* acc_intrinsic;      /* [N] += intrinsic[n], or NULL */
    void* workspace;            /* GF_RND_WORKSPACE_BYTES(N) bytes, 8-byte aligned (required) */
    int64_t workspace_bytes;
} GfRndRewardArgs;

/* ------------------------------------------------------------------------------------------
 * The behaviour-cloning loss of one time step of a distillation update and its gradient (rsl_rl Distillation.update:
 * loss_fn(student mean, stored teacher actions) with loss_type "mse" or "huber", and its backward down to the student's output):
 *     d[n, j] = mu[n, j] - target[n, j]                                      (one rounding)
 *     GF_BC_LOSS_MSE:    e = d²                         grad[n, j] = inv · (2 · d)
 *     GF_BC_LOSS_HUBER:  e = |d| < 1 ? 0.5·d² : |d| - 0.5   grad[n, j] = inv · clamp(d, -1, 1)      (torch's huber_loss, delta 1)
 *     loss = mean over the N·A elements of e   -> out[0] (float32), and sums[0] += (double)out[0] when sums != NULL
 * with inv = 1 / (float)(N·A).  `grad` is WRITTEN, not added to; grad == NULL is the loss-only mode: nothing but out / sums is
 * written.  e is evaluated and summed in double from the f32 d.  The mse form is gf_mirror_loss's operation order with coeff = 1, the
 * identity permutation, sign +1 and a zeroed grad: the two agree bit for bit.
 * The shape of gf_mirror_loss: one lane per row, one double partial per workgroup in the caller's workspace, a second one-workgroup
 * launch sums them in a fixed order.  No atomics: bitwise reproducible.
 * Refusals, before anything is launched: GF_E_NULL — args, mu, target, out, workspace; GF_E_RANGE — num_rows < 0, num_actions < 1,
 * loss_type outside {0, 1}, a workspace smaller than GF_BC_LOSS_WORKSPACE_BYTES(N) or not 8-byte aligned.  num_rows == 0 is a no-op.
 * No allocation, no copy, no synchronisation inside.  Not a phase of the step.
 * ---------------------------------------------------------------------------------------- */
#define GF_BC_LOSS_MSE 0
#define GF_BC_LOSS_HUBER 1
#define GF_BC_LOSS_BLOCK_ROWS 256      /* rows per workgroup of gf_bc_loss: one double partial per workgroup */
#define GF_BC_LOSS_WORKSPACE_BYTES(n) ((int64_t)(((n) + GF_BC_LOSS_BLOCK_ROWS - 1) / GF_BC_LOSS_BLOCK_ROWS) * 8)

typedef struct GfBcLossArgs {
    int64_t num_rows;           /* N >= 0; 0: nothing is launched */
    int32_t num_actions;        /* A >= 1 */
    int32_t loss_type;          /* GF_BC_LOSS_MSE / GF_BC_LOSS_HUBER */
    const float* mu;            /* [N, A] the student's mean of this update */
    const float* target;        /* [N, A] the stored teacher actions (a constant) */
    float* grad;                /* [N, A] = d loss / d mu, or NULL: loss only */
    float* out;                 /* [1] the loss (required) */
    double* sums;               /* [1] += the loss, or NULL */
    void* workspace;            /* GF_BC_LOSS_WORKSPACE_BYTES(N) bytes, 8-byte aligned */
    int64_t workspace_bytes;
} GfBcLossArgs;

/* ------------------------------------------------------------------------------------------
 * Running observation statistics (rsl_rl EmpiricalNormalization.update; the "empirical_normalization" switch of the training
 * scripts, rsl_rl 3.x's actor_obs_normalization / critic_obs_normalization).  rsl_rl updates a normaliser with torch.mean, torch.var
 * and a handful of elementwise launches — about ten per normaliser and collection step.  gf_obs_norm_update updates up to
 * GF_OBS_NORM_MAX_SETS normalisers (the actor's and the critic's) from num_rows rows each in TWO launches.  A set reads its input as
 * up to GF_MLP_MAX_INPUTS segments `[N, width]` side by side (as gf_mlp_act: no torch.cat, `row_stride` floats from row to row), total width W <= GF_MLP_MAX_INPUT_WIDTH.
 * Per set and column c, with N = num_rows:
 *     if until >= 0 and count >= until:  nothing of the set is written
 *     mx = (Σ_n x[n,c]) / N          vx = (Σ_n (x[n,c] - mx)²) / N           (biased, as torch.var(unbiased=False))
 *     count' = count + N             rate = N / count'
 *     d = mx - mean                  mean' = mean + rate·d
 *     var' = var + rate·(vx - var + d·(mx - mean'))
 *     std' = sqrtf(var')             (from the f32-rounded var': torch.sqrt(_var) bit for bit)
 * Everything down to var' is evaluated in float64 from the f32 inputs and the f32 state; mean' and var' are rounded to f32 once each
 * when stored.
 * Launch 1: workgroups own tiles of GF_OBS_NORM_TILE_ROWS rows (at most GF_OBS_NORM_MAX_PARTIALS workgroups per set, grid-stride
 * above); a lane keeps a fixed column (a fixed four above 256 columns) as it walks rows and accumulates Σ(x - s), Σ(x - s)² in float64
 * around s = the first element it reads; a workgroup leaves one record per column — its row count once, then (mean, M2 = Σ(x - mean)²)
 * per column — in the caller's workspace.  Launch 2: ONE workgroup per set sums the records in a fixed order, applies the update and
 * writes mean / var / std / count — the only workgroup that reads or writes `count`.  grid y = set in both launches.  No float atomics,
 * no hand-off or wait between workgroups: bitwise reproducible from run to run, and a column's result does not depend on the other set.
 * Refusals, before anything is launched: GF_E_NULL — args, a segment / mean / var / std / count / workspace pointer; GF_E_RANGE —
 * num_rows < 0, num_sets outside 1 … GF_OBS_NORM_MAX_SETS, a segment count outside 1 … GF_MLP_MAX_INPUTS, a width < 1, a non-zero
 * row_stride < width, a total width > GF_MLP_MAX_INPUT_WIDTH, a workspace smaller than GF_OBS_NORM_WORKSPACE_BYTES(num_rows, W) or not 8-byte aligned, a count pointer
 * not 8-byte aligned.  num_rows == 0 is a no-op.  No allocation, no copy, no synchronisation inside.  Not a phase of the step.
 * ---------------------------------------------------------------------------------------- */
#define GF_OBS_NORM_MAX_SETS 2         /* normalisers per call (actor, critic) */
#define GF_OBS_NORM_TILE_ROWS 256      /* rows per tile of launch 1 */
#define GF_OBS_NORM_MAX_PARTIALS 256   /* workgroups (partial records) per set at most */
#define GF_OBS_NORM_PARTIALS(N) \
    ((((N) + GF_OBS_NORM_TILE_ROWS - 1) / GF_OBS_NORM_TILE_ROWS) < GF_OBS_NORM_MAX_PARTIALS ? \
     (((N) + GF_OBS_NORM_TILE_ROWS - 1) / GF_OBS_NORM_TILE_ROWS) : GF_OBS_NORM_MAX_PARTIALS)
/* workspace of one set: (1 + 2 W) doubles per partial workgroup — {rows, mean[W], M2[W]} — 8-byte aligned */
#define GF_OBS_NORM_WORKSPACE_BYTES(N, W) ((int64_t)GF_OBS_NORM_PARTIALS((int64_t)(N)) * (1 + 2 * (int64_t)(W)) * 8)

typedef struct GfObsNormSet {
    int32_t num_inputs;         /* 1 … GF_MLP_MAX_INPUTS */
    int32_t _pad;
    GfMlpSegment inputs[GF_MLP_MAX_INPUTS];   /* [num_rows, width] each, side by side: W = the sum of the widths */
    float* mean;                /* [W] running mean, updated in place */
    float* var;                 /* [W] running (biased) variance */
    float* std;                 /* [W] sqrt(var) */
    int64_t* count;             /* one word: rows seen so far (rsl_rl's `count` buffer) */
    int64_t until;              /* >= 0: no update once count >= until; negative: none */
    void* workspace;            /* GF_OBS_NORM_WORKSPACE_BYTES(num_rows, W) bytes, 8-byte aligned; not shared with the other set */
    int64_t workspace_bytes;
} GfObsNormSet;

typedef struct GfObsNormArgs {
    int64_t num_rows;           /* N >= 0 rows of every set; 0: nothing is launched */
    int32_t num_sets;           /* 1 … GF_OBS_NORM_MAX_SETS */
    int32_t _pad;
    GfObsNormSet sets[GF_OBS_NORM_MAX_SETS];
} GfObsNormArgs;

/* ------------------------------------------------------------------------------------------
 * History ring -> the reference's observation layout.  The reference keeps a list of H frames, pops the oldest, inserts the new
 * one in front and returns `torch.cat(self._history, dim=-1)` (observation_manager.py:219-226): every call writes a NEW
 * [N, H*O] tensor, newest frame first.  With the history kept as an in-place ring (GfObservationArgs.history_ring: the step
 * writes O floats per env) that returned tensor is one streaming gather: out[n, j*O + c] = ring[n, (k + j) mod H, c] with k the
 * slot of the newest frame.  Unlike shifting the previous output inside the step's kernel, the copy has no dependency on the
 * step's arithmetic and runs as thousands of short workgroups at the copy rate of the memory system; it is also the caller's
 * private tensor, so the default output mode needs no clone on top.
 * ---------------------------------------------------------------------------------------- */
typedef struct GfHistoryUnrollArgs {
    const float* ring;        /* [N, H, O]: the `obs` of launches with history_ring != 0 */
    float* out;               /* [N, H*O], 16-byte aligned */
    float* out2;              /* optional second destination with the same layout (a rollout-storage row), or NULL */
    int64_t num_envs;
    int32_t frame_width;      /* O >= 1 */
    int32_t history_len;      /* H >= 1 */
    int32_t ring_slot;        /* the history_ring value of the launch that wrote the newest frame: k + 1 */
    int32_t _pad;
} GfHistoryUnrollArgs;

/* ------------------------------------------------------------------------------------------
 * Terrain height scan (managers/height_scanner.py; legged_gym's `measured_heights`, Isaac Lab's `height_scan`): the terrain
 * height at P points around each env's base, P body-frame offsets (x forward, y left) shared by every env and turned by the
 * base's yaw.  One launch writes out[n, p] for n < num_envs, p < num_points.  Per element, in f32 with one rounding per operation:
 *     c  = 1 - 2*(qy*qy + qz*qz)        s = 2*(qw*qz + qx*qy)              (the yaw's cosine and sine times cos(pitch))
 *     nrm = sqrt(c*c + s*s)
 *     (cy, sy) = nrm < 1e-6f ? (1, 0) : (c / nrm, s / nrm)                 (align = 0: (1, 0), `quat` is never read)
 *     px = bx + (cy*ox - sy*oy)         py = by + (sy*ox + cy*oy)
 *     h  = the height GfTerrainHeightArgs documents, at (px, py)           (the same device function: the same bits)
 *     v  = relative ? (bz - offset) - h : h
 *     out = min(max(v, clip_lo), clip_hi)                                  (a NaN stays a NaN, as torch.clamp)
 * c, s, nrm, cy, sy and bz - offset are computed once per env.  A 256-lane workgroup owns a tile of GF_HEIGHT_SCAN_TILE_ENVS envs: it
 * stages the pattern and the tile's frames (bx, by, bz - offset, cy, sy) in LDS, then walks the tile's elements with consecutive
 * lanes on consecutive p.  Stores are 16 bytes per lane where `out` is 16-byte aligned and either dense (out_stride == P: a
 * tile's rows are one contiguous run) or made of whole quads (P and out_stride multiples of 4); one float per lane otherwise.
 * The four taps are plain loads (the field is shared by every env and stays in L1 / L2).  No atomics, nothing between workgroups.
 * Refusals, before anything is launched: GF_E_NULL — args, out, pos, pattern, quat with align = 1; GF_E_RANGE — num_envs < 0 (or
 * more than 2^31 - 1 tiles), num_points outside 1 … GF_HEIGHT_SCAN_MAX_POINTS, pos_stride < 3, quat_stride < 4 (with a quat),
 * out_stride < num_points, align / relative outside {0, 1}, clip_lo > clip_hi, a height field with rows < 1 or cols < 1.
 * num_envs == 0 is a no-op.  Runs under GF_PHASE_TERRAIN for gf_profile_begin.  Not a phase of the step.
 * ---------------------------------------------------------------------------------------- */
#define GF_HEIGHT_SCAN_MAX_POINTS 1024
#define GF_HEIGHT_SCAN_TILE_ENVS 16     /* envs per workgroup */

typedef struct GfHeightScanArgs {
    int64_t num_envs;
    const float* pos;          /* row n at pos + n * pos_stride: x, y, z of the base */
    const float* quat;         /* row n at quat + n * quat_stride: w, x, y, z; may be NULL with align = 0 */
    const float* pattern;      /* [P, 2] body-frame offsets */
    float* out;                /* row n at out + n * out_stride, P floats */
    float* points_out;         /* optional [N, P, 2] dense: the world sample points (px, py); NULL: not written */
    int64_t pos_stride;        /* in floats, >= 3 */
    int64_t quat_stride;       /* in floats, >= 4 */
    int64_t out_stride;        /* in floats, >= P */
    GfTerrainView terrain;
    int32_t num_points;        /* P: 1 … GF_HEIGHT_SCAN_MAX_POINTS */
    int32_t align;             /* 0 = world axes, 1 = the base's yaw */
    int32_t relative;          /* 0 = terrain height, 1 = (bz - offset) - terrain height */
    float offset;
    float clip_lo;             /* -inf … */
    float clip_hi;             /* … +inf allowed */
} GfHeightScanArgs;

/* ------------------------------------------------------------------------------------------
 * Terrain ray cast (managers/ray_caster.py; Isaac Lab's RayCaster and its camera, the depth images of the parkour papers): R rays
 * per env against the terrain surface, in one launch.  `pattern` is [R, 6], shared by every env: a body-frame start offset p and a
 * UNIT direction e per ray (the host normalises in f64 and rounds once; the kernel never normalises).
 *
 * Surface.  Inside the field's rectangle [x_min, x_min + x_span] x [y_min, y_min + y_span] it is S(x, y), the bilinear interpolant
 * of the cell's four corners at grid coordinates gx = (x - x_min) * sx, gy = (y - y_min) * sy with sx = (float)(cols - 1) / x_span,
 * sy = (float)(rows - 1) / y_span.  Outside the rectangle there is no surface: a ray passes (the border clamp of the height
 * sampler is NOT extended).  height_field == NULL: the plane z = origin_z everywhere.
 * Result.  t* = the smallest t in [0, max_range] whose point lies in the rectangle with oz + t*dz <= S; none: the ray misses.
 * out[n, r] = t* (mode 0, distance) or t* * ((ex*ax + ey*ay) + ez*az) (mode 1, depth along the body-frame optical axis `axis`);
 * a miss writes miss_value (any float).  hits_out[n, r] = o + te*d with te = t* for a hit, max_range for a miss.
 *
 * In f32, one rounding per operation (never fused), `x ? a : b` selects written out so that a NaN takes the same side everywhere:
 *   frame, once per env —
 *     align 2 (base): the rotation matrix of the quaternion as given (not normalised)
 *       r00 = 1 - 2*(qy*qy + qz*qz)   r01 = 2*(qx*qy - qw*qz)        r02 = 2*(qx*qz + qw*qy)
 *       r10 = 2*(qw*qz + qx*qy)       r11 = 1 - 2*(qx*qx + qz*qz)    r12 = 2*(qy*qz - qw*qx)
 *       r20 = 2*(qx*qz - qw*qy)       r21 = 2*(qy*qz + qw*qx)        r22 = 1 - 2*(qx*qx + qy*qy)
 *     align 1 (yaw): (cy, sy) exactly as the height scan computes them (c = r00, s = r10 above); rows (cy, -sy, 0), (sy, cy, 0), (0, 0, 1)
 *     align 0 (world): the identity; `quat` is never read
 *   ray —
 *     ox = bx + ((r00*px + r01*py) + r02*pz)   (oy, oz with rows 1, 2)      dx = (r00*ex + r01*ey) + r02*ez   (dy, dz likewise)
 *   plane (no height field) —
 *     C = oz - origin_z;  C <= 0: hit, t* = 0;  else dz < 0 and tt = C / (-dz) <= max_range: hit, t* = tt;  else miss
 *   field —
 *     gx0 = (ox - x_min)*sx   du = dx*sx   idu = 1/du        (y: gy0, dv, idv with y_min, sy)       fw = (float)(cols-1), fh likewise
 *     slab: t0 = 0, t1 = max_range; per axis, if du != 0: ta = (-gx0)*idu, tb = (fw - gx0)*idu, lo = ta < tb ? ta : tb,
 *       hi = ta < tb ? tb : ta, if (lo > t0) t0 = lo, if (hi < t1) t1 = hi; if du == 0 the ray needs 0 <= gx0 <= fw.  Miss unless t0 <= t1.
 *     entry: tin = t0; gin = gx0 + tin*du; ix = (int)floor(gin), minus 1 if du < 0 and gin == floor(gin) (a start on a grid line
 *       heading in the negative direction belongs to the cell behind the line); ix clamped to 0 … cols-2.  iy likewise.
 *     walk, at most (cols-1) + (rows-1) + 1 cells:
 *       tnx = du != 0 ? ((float)(ix + (du > 0)) - gx0)*idu : +inf        tny likewise        tn = tnx < tny ? tnx : tny
 *       tout = tn < t1 ? tn : t1;  tout = tout > tin ? tout : tin;  smax = tout - tin
 *       u0 = (gx0 + tin*du) - (float)ix, clamped to [0, 1] (< 0 first, then > 1)       v0 likewise       zin = oz + tin*dz
 *       h00 = f[iy][ix]  h10 = f[iy][ix+1]  h01 = f[iy+1][ix]  h11 = f[iy+1][ix+1]
 *       a = h10 - h00    b = h01 - h00    k = (h00 - h10) - (h01 - h11)
 *       C = zin - (((h00 + a*u0) + b*v0) + (k*u0)*v0)
 *       B = dz - ((a*du + b*dv) + k*(u0*dv + v0*du))
 *       A = -((k*du)*dv)                                   (the gap along the ray inside the cell is C + B*s + A*s*s, s = t - tin)
 *       C <= 0: hit at t* = tin (an origin under the surface gives 0).  Otherwise s = +inf and
 *         A == 0: if B < 0, s = C / (-B)
 *         A != 0: disc = B*B - (4*A)*C; if disc >= 0: sq = sqrt(disc), q = -0.5*(B + (B < 0 ? -sq : sq)), r1 = q / A, r2 = C / q,
 *                 if (r1 >= 0 && r1 < s) s = r1, if (r2 >= 0 && r2 < s) s = r2           (the cancellation-free pair of roots)
 *       s <= smax: hit at t* = tin + s.  Otherwise, unless tn < t1, the ray ended: miss.  Else step: if (tnx <= tn) ix += sign(du),
 *       if (tny <= tn) iy += sign(dv) (a tie steps both; one index always steps, also when rounding put tn at or before tin); an
 *       index outside 0 … cols-2 / 0 … rows-2: miss; tin = tout.
 * A 256-lane workgroup owns a tile of GF_RAY_CAST_TILE_ENVS envs: the frames (origin and nine matrix entries) and the pattern are
 * staged in LDS, consecutive lanes take consecutive rays, stores are 16 bytes wide under the height scan's rule (out 16-byte aligned
 * and dense, or num_rays and out_stride multiples of 4).  The taps are plain loads.  No atomics, nothing between workgroups.
 * Refusals, before anything is launched: GF_E_NULL — args, out, pos, pattern, quat with align != 0; GF_E_RANGE — num_envs < 0 (or
 * more than 2^31 - 1 tiles), num_rays outside 1 … GF_RAY_CAST_MAX_RAYS, pos_stride < 3, quat_stride < 4 (with a quat),
 * out_stride < num_rays, align outside {0, 1, 2}, mode outside {0, 1}, max_range negative or not finite, a height field with
 * rows < 2 or cols < 2.  num_envs == 0 is a no-op.  Runs under GF_PHASE_TERRAIN for gf_profile_begin.  Not a phase of the step.
 * ---------------------------------------------------------------------------------------- */
#define GF_RAY_CAST_MAX_RAYS 2048       /* a 64 x 32 image */
#define GF_RAY_CAST_TILE_ENVS 8         /* envs per workgroup */
enum { GF_RAY_ALIGN_WORLD = 0, GF_RAY_ALIGN_YAW = 1, GF_RAY_ALIGN_BASE = 2 };
enum { GF_RAY_MODE_DISTANCE = 0, GF_RAY_MODE_DEPTH = 1 };

typedef struct GfRayCastArgs {
    int64_t num_envs;
    const float* pos;          /* row n at pos + n * pos_stride: x, y, z of the base */
    const float* quat;         /* row n at quat + n * quat_stride: w, x, y, z; may be NULL with align = 0 */
    const float* pattern;      /* [R, 6]: px, py, pz, ex, ey, ez */
    float* out;                /* row n at out + n * out_stride, R floats */
    float* hits_out;           /* optional [N, R, 3] dense: the world hit points; NULL: not written */
    int64_t pos_stride;        /* in floats, >= 3 */
    int64_t quat_stride;       /* in floats, >= 4 */
    int64_t out_stride;        /* in floats, >= R */
    GfTerrainView terrain;
    int32_t num_rays;          /* R: 1 … GF_RAY_CAST_MAX_RAYS */
    int32_t align;             /* GF_RAY_ALIGN_* */
    int32_t mode;              /* GF_RAY_MODE_* */
    float axis[3];             /* the optical axis in the body frame (mode 1) */
    float max_range;           /* finite, >= 0 */
    float miss_value;
} GfRayCastArgs;

/* ------------------------------------------------------------------------------------------
 * Terrain curriculum (managers/terrain_curriculum.py, mdp.reset.terrain_curriculum_position; legged_gym's
 * _update_terrain_curriculum, Isaac Lab's terrain_levels_vel): the terrain is a grid of cells, difficulty growing along one axis;
 * every env owns a (level, type) cell and respawns inside it.  One launch does the whole reset of the base for the flagged envs —
 * level change, draws, position with the terrain height, orientation, velocities, bookkeeping.  For env n with
 * mask[n] || (mask2 && mask2[n]), in f32 with one rounding per operation, in this order:
 *   1. dx = pos_in[3n] - spawn_xy[2n], dy likewise; dist = sqrt(dx*dx + dy*dy)            (the distance walked since the spawn)
 *   2. only if update != 0:  up = dist > promote_distance  (strict);  thr = speed_ref ? speed_ref[n] * demote_time : demote_distance;
 *      down = !up && dist < thr;  l = level[n] + up - down.       With update == 0: l = level[n], and steps 1 and 4 are skipped.
 *   3. draws u[0..5] = (x, y, rot x, rot y, rot z, level): row n of the dense `draws` [N, 6], or, with draws == NULL, Philox with
 *      counter n + env_offset of `stream`: block GF_SPAWN_BLOCK gives (u0, u1, u4, u5), block GF_SPAWN_BLOCK + 1 gives (u2, u3) and is
 *      computed only when spawn_rot_mask & 3 (else u2 = u3 = 0) — the spawn draws of GfResetArgs, plus the fourth word of the first
 *      block, which that layout leaves unused.
 *   4. l >= num_levels: l = min((int)(u5 * (float)num_levels), num_levels - 1), counted as a wrap.  Then l < 0: l = 0.
 *   5. (ix, iy) = level_axis == 0 ? (l, type[n]) : (type[n], l)
 *   6. x = (u0 * spawn_x_span + spawn_x_min) + (float)ix * cell_dx;  y likewise with u1, iy, cell_dy.  spawn_* is the usable rectangle
 *      of cell (0, 0), computed by the host in double and stored as f32.  z = the height GfTerrainHeightArgs documents at (x, y)
 *      (the same device function: the same bits) + height_offset.
 *   7. set_quat: angle k = bit k of spawn_rot_mask ? u[2 + k] * (spawn_rot_hi[k] - spawn_rot_lo[k]) + spawn_rot_lo[k] : 0, the
 *      quaternion by the deterministic xyz_to_quat of GfResetArgs' spawn.
 *   8. writes: pos_out[n]; quat_out[n] if set_quat (the old quat_out[n] goes to quat_stash[n] first when quat_stash is given); zeros
 *      to lin_vel, ang_vel, dof_vel [N, num_dofs] where non-NULL and zero_velocity is set; spawn_xy[n] = (x, y); level[n] = l;
 *      if command.command: speed_ref[n] = sqrt(cx*cx + cy*cy) of the command's first two columns (stored after step 2 read the old
 *      value); counts[0..2] += promoted (up), demoted (down, also when the floor of step 4 kept the level), wrapped.
 * An env that is not flagged has nothing of its own written.  pos_in and pos_out may be the same buffer (a lane reads its row
 * before it writes it).  A lane owns an env; a wave without a flagged lane leaves after the ballot; the counters are one vector
 * atomicAdd per wave and counter; no LDS, nothing between workgroups.  A workgroup holds GF_TERRAIN_CURRICULUM_BLOCK_ENVS envs.
 * Refusals, before any HIP call: GF_E_NULL — args, mask, pos_in, pos_out, spawn_xy, level, type, counts, quat_out with set_quat,
 * speed_ref with a command; GF_E_RANGE — num_envs < 0 (or more than 2^31 - 1 workgroups), num_levels < 1, num_types < 1,
 * num_dofs < 0, level_axis / update / set_quat outside {0, 1}, promote_distance / demote_time / demote_distance negative or not
 * finite, a height field with rows < 1 or cols < 1, a command with width < 2 (or 0 < stride < width); GF_E_UNSUPPORTED — quat_out
 * or quat_stash not 16-byte aligned (a row moves as one unit).  num_envs == 0 is a no-op.  Runs under GF_PHASE_TERRAIN for
 * gf_profile_begin.  Not a phase of the step.
 * ---------------------------------------------------------------------------------------- */
#define GF_TERRAIN_CURRICULUM_BLOCK_ENVS 256   /* envs per workgroup (four waves) */

typedef struct GfTerrainCurriculumArgs {
    int64_t num_envs;
    const uint8_t* mask;       /* [N] one byte per env */
    const uint8_t* mask2;      /* [N] or NULL: OR-ed with mask */
    const float* pos_in;       /* [N,3] the base position the episode ended at */
    float* pos_out;            /* [N,3] the spawn position; may be pos_in */
    float* quat_out;           /* [N,4] 16-byte aligned; may be NULL with set_quat = 0 */
    float* quat_stash;         /* [N,4] 16-byte aligned or NULL: receives the pre-reset quat_out rows */
    float* lin_vel;            /* [N,3] or NULL */
    float* ang_vel;            /* [N,3] or NULL */
    float* dof_vel;            /* [N,num_dofs] or NULL */
    float* spawn_xy;           /* [N,2] where each env last spawned: read, then rewritten */
    int32_t* level;            /* [N] read, then rewritten */
    const int32_t* type;       /* [N] */
    float* speed_ref;          /* [N] or NULL (then demote_distance is the threshold) */
    int32_t* counts;           /* [3] promoted, demoted, wrapped: added to */
    const float* draws;        /* [N,6] U[0,1) or NULL -> Philox */
    GfCommandView command;     /* .command NULL: speed_ref is not rewritten */
    uint64_t seed;
    uint64_t stream;
    uint32_t env_offset;
    int32_t num_dofs;
    int32_t num_levels;
    int32_t num_types;
    int32_t level_axis;        /* 0: levels along x, types along y; 1: the other way round */
    int32_t update;            /* 0: respawn in the current cell; 1: move levels first */
    int32_t set_quat;
    int32_t zero_velocity;
    int32_t spawn_rot_mask;
    float promote_distance;
    float demote_time;
    float demote_distance;
    float spawn_x_min, spawn_x_span, spawn_y_min, spawn_y_span;   /* the usable rectangle of cell (0, 0) */
    float cell_dx, cell_dy;    /* the cell pitch */
    float height_offset;
    float spawn_rot_lo[3], spawn_rot_hi[3];
    GfTerrainView terrain;
} GfTerrainCurriculumArgs;

/* ------------------------------------------------------------------------------------------
 * Random pushes (managers/push.py; legged_gym's push_robots / _push_robots, Isaac Lab's push_by_setting_velocity as an `interval`
 * event): every few seconds the base gets a random velocity.  One launch keeps the per-env interval timers and gives the kick.
 * The state is due[n], the value of `step` (the push's own call counter, uint32, wrapping) at which env n is pushed next — an
 * absolute step, not a countdown, so that a launch in which nothing happens writes nothing but `fired`.  For env n, in this order
 * (f32 with one rounding per operation, nothing contracted; integer sums modulo 2^32):
 *   1. done = !global_timer && ((mask && mask[n]) || (mask2 && mask2[n]))         (this step's terminated / truncated masks)
 *   2. fire = !done && (int32)(step - (uint32)due[n]) >= 0                         (wrap-safe: true for up to 2^31 - 1 steps past due)
 *   3. if done || fire:  W = interval_hi - interval_lo + 1;
 *      due[n] = (int32)(step + interval_lo + min((int)(u3 * (float)W), W - 1))
 *   4. if fire, for every component j with bit j of comp_mask set (0..2: lin_vel x, y, z; 3..5: ang_vel x, y, z):
 *      v = (u_j * (hi[j] - lo[j]) + lo[j]) * scale;  mode 0: vel[j] = v;  mode 1: vel[j] = vel[j] + v.
 *      A component whose bit is clear is neither read nor written.
 *   5. fired[n] = fire (where fired is given: written for EVERY env); counts[0] += the number of envs that fired.
 * An env that finished its episode in this step is not pushed: it gets a fresh timer (Isaac Lab's per-env interval rule).  With
 * global_timer the masks are not looked at (they may be NULL) and every env is pushed in the same steps (legged_gym).
 * Draws: row n of the dense `draws` [N, 7] = (u0 … u6) (parity mode; with global_timer the caller puts the same u3 into every row),
 * or, with draws == NULL, Philox4x32-10 keyed by seed ^ GF_PUSH_SEED_TAG — a key of its own, so no counter of any other phase can
 * coincide — with counter (n + env_offset, block, step, 0), words to floats by u24_to_unit: block 0 gives (u0, u1, u2, u3), block 1
 * gives (u4, u5, u6, -) and is computed only when comp_mask & 0x38.  With global_timer u3 is the fourth word of the block with
 * counter (0xFFFFFFFF, 0, step, 0) instead: the same for every env, on every rank.
 * A lane owns an env; a wave in which no lane is done or fires leaves after the ballot, having written its `fired` bytes — with
 * intervals of hundreds of steps that is what almost every wave does; counts takes one vector atomicAdd per wave; no LDS, nothing
 * between workgroups.  A workgroup holds GF_PUSH_BLOCK_ENVS envs.
 * Refusals, before any HIP call: GF_E_NULL — args, due, lin_vel, counts, ang_vel with comp_mask & 0x38; GF_E_RANGE — num_envs < 0
 * (or more than 2^31 - 1 workgroups), not 1 <= interval_lo <= interval_hi, interval_hi - interval_lo + 1 > 2^24 (u3 has 24 bits),
 * mode / global_timer outside {0, 1}, comp_mask outside 0 … 63, a lo[j], hi[j] or scale that is not finite, hi[j] < lo[j] on an
 * enabled component.  num_envs == 0 is a no-op.  Runs under GF_PHASE_TERRAIN for gf_profile_begin (the rough-terrain task's other
 * additive entries do).  Not a phase of the step.
 * ---------------------------------------------------------------------------------------- */
#define GF_PUSH_BLOCK_ENVS 256                     /* envs per workgroup (four waves) */
#define GF_PUSH_SEED_TAG 0x9D15B0057ED5EEDBull     /* XOR-ed into the seed of the push draws: a key of its own */

typedef struct GfPushArgs {
    int64_t num_envs;
    const uint8_t* mask;       /* [N] one byte per env, or NULL */
    const uint8_t* mask2;      /* [N] or NULL: OR-ed with mask */
    int32_t* due;              /* [N] the step at which the env is pushed next: read, rewritten where done or fired */
    float* lin_vel;            /* [N,3] */
    float* ang_vel;            /* [N,3]; may be NULL when comp_mask & 0x38 == 0 */
    uint8_t* fired;            /* [N] or NULL: 1 where pushed, 0 elsewhere */
    int32_t* counts;           /* [1] pushes: added to */
    const float* draws;        /* [N,7] U[0,1) or NULL -> Philox */
    uint64_t seed;             /* Philox key = seed ^ GF_PUSH_SEED_TAG */
    uint32_t step;             /* the push's own call counter */
    uint32_t env_offset;
    int32_t interval_lo;       /* steps, 1 <= interval_lo <= interval_hi */
    int32_t interval_hi;
    int32_t mode;              /* 0: set the enabled components; 1: add to them */
    int32_t comp_mask;         /* bits 0..2: lin x, y, z; bits 3..5: ang x, y, z */
    int32_t global_timer;      /* 0: per-env timers; 1: one interval draw for every env, masks ignored */
    float lo[6], hi[6];        /* the range of each component */
    float scale;               /* multiplies every drawn velocity (a magnitude curriculum) */
} GfPushArgs;

/* ------------------------------------------------------------------------------------------
 * Actuator latency (managers/action_delay.py; Isaac Lab's DelayedPDActuator with its per-env DelayBuffer, the "action lag" buffer of
 * the legged_gym forks): the position targets a policy commands reach the actuators lag[n] control steps late, and the lag is drawn
 * per env and per episode.  One launch writes this step's targets into a ring of `slots` = L steps, hands out the targets of
 * lag[n] steps ago and re-draws the lag and primes the ring of every env whose episode has just begun.
 * ring is [L, N, D], slot-major: the write to slot `head` is one coalesced stream, a lagged read a contiguous D-row of another slot.
 * `head` is the slot this call writes; the host advances it by one modulo L per call (it is not derived from the wrapping call
 * counter `step`: L need not divide 2^32).  For env n, in this order:
 *   1. fresh = prime_all || (episode_length && episode_length[n] <= 1) || (mask && mask[n]) || (mask2 && mask2[n])
 *      (episode_length is the env's counter AFTER this step's increment: 1 in the first step of an episode, 0 where a reset ran and
 *      no step has; every input of the test is read-only in the launch, so all lanes that own a part of the env decide alike)
 *   2. fresh:  u = draws ? draws[n] : u24_to_unit(x word of Philox4x32-10, counter (n + env_offset, 0, step, 0),
 *                                                  key seed ^ GF_ACTION_DELAY_SEED_TAG);
 *              W = lag_hi - lag_lo + 1;  lag[n] = lag_lo + min((int)(u * (float)W), W - 1)        (one f32 product, truncated)
 *   3. fresh:  ring[s, n, :] = in[n, :] for every s in 0 … L-1;  out[n, :] = in[n, :]
 *      (Isaac Lab's rule: a cleared buffer is filled with the first value pushed, so a new episode sees its own command until the
 *      history exists.  A lane that does not write lag[n] computes the draw again; it never reads lag[n] back.)
 *   4. otherwise:  ring[head, n, :] = in[n, :];  l = lag[n];
 *              out[n, :] = l == 0 ? in[n, :] : ring[(head + L - l) % L, n, :]                     (never the slot just written)
 *      lag[n] is not written, nor is any slot but `head`.  A lag[n] outside 0 … L-1 (state the launch did not write) reads as 0.
 *   5. Values move as bits: a NaN or Inf of `in` arrives in `out` lag[n] steps later with the same bit pattern.
 * The [N, D] streams move as 16-byte words, one per lane, when D % 4 == 0 and in / out / ring are 16-byte aligned (a word is then
 * four DOFs of one env), element by element otherwise; no LDS, nothing between lanes.  Traffic of an ordinary step: 16 D bytes per
 * env (in, the slot written, the slot read, out) + 4 of lag + the freshness bytes.
 * Refusals, before any HIP call: GF_E_NULL — args, in, out, ring, lag; GF_E_RANGE — num_envs < 0 (or more than 2^31 - 1
 * workgroups), num_dofs <= 0, slots outside 1 … GF_ACTION_DELAY_MAX_SLOTS, head outside 0 … slots-1, not
 * 0 <= lag_lo <= lag_hi <= slots-1, prime_all outside {0, 1}.  num_envs == 0 is a no-op.  Runs under GF_PHASE_TERRAIN for
 * gf_profile_begin (the rough-terrain task's other additive entries do).  Not a phase of the step.
 * ---------------------------------------------------------------------------------------- */
#define GF_ACTION_DELAY_MAX_SLOTS 64                       /* the ring's capacity: the largest lag is 63 steps */
#define GF_ACTION_DELAY_SEED_TAG 0xAC7DE1A7C0FFEE5Dull     /* XOR-ed into the seed of the lag draws: a key of its own */

typedef struct GfActionDelayArgs {
    int64_t num_envs;
    const float* in;           /* [N,D] this step's targets */
    float* out;                /* [N,D] the targets the actuators get */
    float* ring;               /* [L,N,D] slot-major history */
    int32_t* lag;              /* [N] steps of delay: read, rewritten where fresh */
    const int32_t* episode_length;   /* [N] or NULL: fresh where <= 1 */
    const uint8_t* mask;       /* [N] one byte per env, or NULL: fresh where set */
    const uint8_t* mask2;      /* [N] or NULL: OR-ed with mask */
    const float* draws;        /* [N] U[0,1) or NULL -> Philox */
    uint64_t seed;             /* Philox key = seed ^ GF_ACTION_DELAY_SEED_TAG */
    uint32_t step;             /* the delay's own call counter */
    uint32_t env_offset;
    int32_t num_dofs;          /* D */
    int32_t slots;             /* L = the largest lag + 1 */
    int32_t head;              /* the slot this call writes */
    int32_t lag_lo;            /* 0 <= lag_lo <= lag_hi <= slots - 1 */
    int32_t lag_hi;
    int32_t prime_all;         /* 1: every env is fresh (the first call, a reset of everything) */
} GfActionDelayArgs;

/* ------------------------------------------------------------------------------------------
 * Entry points.  `stream` is a hipStream_t (torch.cuda.current_stream().cuda_stream).
 * ---------------------------------------------------------------------------------------- */
int gf_abi_version(void);
/* library-wide tuning switches (process global).  GF_OPT_POST_VARIANT selects the fused post-physics kernel:
 * 1 = table interpreter (four specialised waves per 64-env tile); 2 = (default) as 1, plus the static programs: a
 * config whose structure matches a registered program runs straight-line code compiled for it.  0 selected a first
 * version of the kernel that is gone: the value stays accepted and means 1.  All variants produce bit-identical results. */
/* GF_OPT_PROFILE_STRIDE: gf_profile_begin stamps every k-th launch of the profiled phase (default 1 = every launch); a
 * stamped launch costs the host several microseconds more than a plain one, so a timed region samples instead. */
/* GF_OPT_GRAPH (default 0): 1 = gf_run_ops_graph replays a recorded step as one hipGraphLaunch.  Off by default because it
 * MEASURED slower on MI355X / ROCm 7.2 (every node's arguments change every step, so each replay pays one
 * hipGraphExecKernelNodeSetParams per kernel on top of the graph launch): Go2 command config 21.7 vs 18.1 µs/step at 4 096
 * envs, 27.8 vs 24 µs at 65 536; gait config 107 vs 94 µs at 8 192 (profiles/r01_l_graph_vs_plain.jsonl). */
/* GF_OPT_CHAIN (default 1): gf_run_ops folds runs of per-env phases the fused post-physics kernel does not cover into phase
 * chains — termination → reward → command.step…, and reset → command.reset… → observe… — one launch each (csrc/gf_chain.hip). */
/* GF_OPT_FOLD_CONTACT (default 1): gf_run_ops hands the contact_step ops in front of a fused post-physics op to that launch
 * (gf_post_physics_step_contacts) instead of launching the contact kernel itself — unless that measured slower (more than 4 tracked
 * links below 16 384 envs, more than 12 below 32 768); 0 keeps the two launches (A/B, tests), 2 folds whenever it is possible. */
enum { GF_OPT_POST_VARIANT = 0, GF_OPT_PROFILE_STRIDE = 1, GF_OPT_GRAPH = 2, GF_OPT_CHAIN = 3, GF_OPT_FOLD_CONTACT = 4, GF_OPT_COUNT = 5 };
int gf_set_option(int option, int value);
int gf_sizeof(int which);   /* sizeof of the ABI structs (0 = GfStepStats … 11 = GfObsItem, 12 GfTerrainView, 13 GfTerrainHeightArgs, 14 GfGaitArgs, 15 GfContactView, 16 GfCommandView, 17 GfPostRefs, 18 GfRolloutArgs, 19 GfHistoryUnrollArgs, 20 GfRolloutPolicyArgs, 21 GfGaeArgs, 22 GfCompactArgs, 23 GfMinibatchArgs, 24 GfPolicyActArgs, 25 GfEpisodeArgs, 26 GfPpoLossArgs, 27 GfAdamArgs, 28 GfMlpActArgs, 29 GfObsNormArgs, 30 GfRolloutFrameArgs, 31 GfMirrorRowsArgs, 32 GfMirrorLossArgs, 33 GfMlpDistillArgs, 34 GfBcLossArgs, 35 GfRndRewardArgs, 36 GfMlpRecurrentActArgs, 37 GfRnnCell, 38 GfTrajTableArgs, 39 GfTrajGatherArgs, 40 GfMlpRecurrentDistillArgs): binding self-check */
const char* gf_build_info(void);
const char* gf_error_string(int code);

int gf_stats_clear(GfStepStats* stats, void* stream);            /* zero all GF_STATS_SHARDS blocks */

int gf_action_step(const GfActionArgs* a, void* stream);          /* replaces genesis_env.py:181-205 + position_action_manager.py:376-419 */
int gf_contact_step(const GfContactArgs* a, void* stream);        /* replaces contact_manager.py:331-336 (+ contact/kernel.py:5-90) */
int gf_termination_step(const GfTerminationArgs* a, void* stream);/* replaces termination_manager.py:151-190 */
int gf_reward_step(const GfRewardArgs* a, void* stream);          /* replaces reward_manager.py:166-195 */
int gf_command_step(const GfCommandArgs* a, void* stream);        /* replaces command_manager.py:152-170,290-303 */
int gf_gait_step(const GfGaitArgs* a, void* stream);              /* replaces examples/gait_trainer/gait_command_manager.py:185-255 */
int gf_masked_reset(const GfResetArgs* a, void* stream);          /* replaces managed_env.py:336-366 fan-out */
int gf_observe(const GfObservationArgs* a, void* stream);         /* replaces observation_manager.py:218-256 */
int gf_entity_rotate(const GfRotateArgs* a, void* stream);        /* replaces entity_manager.py:130-146 */
int gf_terrain_height(const GfTerrainHeightArgs* a, void* stream);/* replaces terrain_manager.py:100-166 */
int gf_height_scan(const GfHeightScanArgs* a, void* stream);     /* the terrain height at P points around every base, yaw-aligned, in one launch (legged_gym measured_heights, Isaac Lab height_scan) */
int gf_height_scan_sizeof(void);                                 /* sizeof(GfHeightScanArgs): the binding's self-check for this additive entry (gf_sizeof's table ends at 40) */
int gf_ray_cast(const GfRayCastArgs* a, void* stream);           /* R rays per env against the terrain surface, exact cell walk, in one launch (Isaac Lab RayCaster / depth camera) */
int gf_ray_cast_sizeof(void);                                    /* sizeof(GfRayCastArgs): the binding's self-check for this additive entry */
int gf_terrain_curriculum(const GfTerrainCurriculumArgs* a, void* stream);   /* promote / demote / respawn of the flagged envs in their terrain cells, in one launch (legged_gym _update_terrain_curriculum, Isaac Lab terrain_levels_vel) */
int gf_terrain_curriculum_sizeof(void);                          /* sizeof(GfTerrainCurriculumArgs): the binding's self-check for this additive entry */
int gf_push(const GfPushArgs* a, void* stream);                  /* per-env interval timers and the random velocity kick of the envs that are due, in one launch (legged_gym _push_robots, Isaac Lab push_by_setting_velocity) */
int gf_push_sizeof(void);                                        /* sizeof(GfPushArgs): the binding's self-check for this additive entry */
int gf_action_delay(const GfActionDelayArgs* a, void* stream);  /* per-env delayed position targets: ring write, lagged read, re-draw and priming of the fresh envs, in one launch (Isaac Lab DelayedPDActuator, legged_gym action lag) */
int gf_action_delay_sizeof(void);                                /* sizeof(GfActionDelayArgs): the binding's self-check for this additive entry */
int gf_synth_scene_step(const GfSynthSceneArgs* a, void* stream); /* stands in for scene.step() (managed_env.py:292) */
int gf_rollout_write(const GfRolloutArgs* a, void* stream);       /* replaces the RolloutStorage copy_ launches of the RL library (examples/simple/train.py:125-129) */
int gf_rollout_frame_write(const GfRolloutFrameArgs* a, void* stream);   /* the newest frame of up to four history observations into a frame-major rollout storage, one launch */
int gf_history_unroll(const GfHistoryUnrollArgs* a, void* stream);/* replaces the torch.cat of observation_manager.py:226 */
int gf_rollout_policy_write(const GfRolloutPolicyArgs* a, void* stream);   /* the policy's rows of a transition + time-out bootstrap (rsl_rl add_transitions; call site examples/simple/train.py:125-129) */
int gf_done_compact(const GfCompactArgs* a, void* stream);       /* replaces the nonzero() of managed_env.py:308-310 where an index list is still needed */
int gf_gae(const GfGaeArgs* a, void* stream);                     /* returns and advantages of a finished rollout (rsl_rl compute_returns; gamma / lam: examples/simple/train.py:41-47) */
int gf_minibatch_gather(const GfMinibatchArgs* a, void* stream);  /* every field of one PPO minibatch in one launch (rsl_rl mini_batch_generator) */
int gf_policy_act(const GfPolicyActArgs* a, void* stream);       /* Normal sample + log_prob + the policy's storage rows in one launch (rsl_rl PPO.act) */
int gf_episode_step(const GfEpisodeArgs* a, void* stream);       /* time-out bootstrap + the runner's rewbuffer / lenbuffer upkeep (rsl_rl OnPolicyRunner.learn) */
int gf_ppo_loss(const GfPpoLossArgs* a, void* stream);           /* minibatch loss + its gradient w.r.t. mu / value / sigma (rsl_rl PPO.update: the KL block, surrogate, value loss, loss, loss.backward() down to the policy outputs, the three .item()) */
int gf_mirror_rows(const GfMirrorRowsArgs* a, void* stream);     /* originals + mirrored copies of up to four row fields, and the replicated per-row scalars, in one launch (rsl_rl PPO.update: data_augmentation_func, torch.cat, repeat) */
int gf_mirror_loss(const GfMirrorLossArgs* a, void* stream);     /* symmetry loss and its gradient w.r.t. the mirrored rows' mu (rsl_rl PPO.update: MSELoss(mean_actions[mb:], mirrored mean_actions[:mb].detach()) and its backward) */
int gf_mlp_act(const GfMlpActArgs* a, void* stream);             /* actor + critic MLP forward on the f32 matrix cores, then gf_policy_act's sampling and rows, in one launch (rsl_rl ActorCritic.act / evaluate inside PPO.act) */
int gf_mlp_recurrent_act(const GfMlpRecurrentActArgs* a, void* stream); /* gf_mlp_act with an LSTM / GRU cell in front of each MLP, the hidden state read and advanced in place, in one launch (rsl_rl ActorCriticRecurrent.act / evaluate inside PPO.act) */
int gf_traj_table(const GfTrajTableArgs* a, void* stream);       /* the trajectories of a rollout: per-env counts, their prefix sum and (env, t0, len), once per update (rsl_rl split_and_pad_trajectories) */
int gf_traj_gather(const GfTrajGatherArgs* a, void* stream);     /* one minibatch of trajectories: padded normalised observations, masks, the un-pad index and the initial states in one launch (rsl_rl recurrent_mini_batch_generator) */
int gf_mlp_distill_act(const GfMlpDistillArgs* a, void* stream); /* student + teacher MLP forward in one launch, the student sampled by gf_policy_act's row code (rsl_rl Distillation.act: StudentTeacher.act / evaluate) */
int gf_mlp_recurrent_distill_act(const GfMlpRecurrentDistillArgs* a, void* stream); /* gf_mlp_distill_act with an LSTM / GRU cell in front of the student's MLP, optionally the teacher's, the hidden states read and advanced in place, in one launch (rsl_rl Distillation.act on a StudentTeacherRecurrent) */
int gf_bc_loss(const GfBcLossArgs* a, void* stream);             /* behaviour-cloning loss of one time step (mse / huber) and its gradient w.r.t. the student's mean (rsl_rl Distillation.update: loss_fn(actions, privileged_actions) and its backward) */
int gf_rnd_reward(const GfRndRewardArgs* a, void* stream);       /* target + predictor MLP forward, their distance, the reward normaliser and the storage row's add in one launch (two with the normaliser updating) (rsl_rl RandomNetworkDistillation.get_intrinsic_reward inside PPO.process_env_step) */
int gf_obs_norm_update(const GfObsNormArgs* a, void* stream);    /* running mean / var / std / count of up to two observation normalisers in two launches (rsl_rl EmpiricalNormalization.update) */
int gf_adam_step(const GfAdamArgs* a, void* stream);             /* adaptive lr + clip_grad_norm_ + Adam.step over the flat bucket (rsl_rl PPO.update: the lr schedule, nn.utils.clip_grad_norm_, optimizer.step()) */

/* ------------------------------------------------------------------------------------------
 * Fused post-physics step: everything ManagedEnvironment.step() does after scene.step() and the
 * contact managers — termination → reward → command.step → reset of done envs → command.reset →
 * observations (managed_env.py:303-326) — as ONE launch.  All of it is per-env work on the same
 * state (pos/quat/vel/ang, the [N,D] rows, commands), so one workgroup carries a 64-env tile through every
 * phase with that state in registers: 566 B/env of traffic instead of 268 + 26 + 4 + 388 + the reset's
 * re-reads, one launch instead of six.  The descriptors are the per-phase ones (so the semantics are by
 * definition those of calling the phases in sequence — which is what the oracle twin does); the call
 * packs them into one kernarg block.  Returns GF_E_UNSUPPORTED when the combination cannot be fused
 * (host-evaluated columns without GF_POST_TERMINATION_DONE — see below —, host-evaluated observation items, parity-mode draws,
 * more than 32 DOF, phases reading different buffers, more than 2 command / 1 gait /
 * 2 observation managers …): the caller then runs the phases one by one (or leaves a manager out of the call and runs it behind).
 * ---------------------------------------------------------------------------------------- */
#define GF_POST_MAX_CMD 2
#define GF_POST_MAX_OBS 2
#define GF_POST_MAX_GAIT 1

/* GfPostRefs.flags.  GF_POST_TERMINATION_DONE: the termination phase of this step has ALREADY run as a launch of its own
 * (gf_termination_step on `termination`: masks and statistics are final) — the fused launch reads `terminated` / `truncated`
 * instead of evaluating the terms.  This is how a step whose task config carries Python-level terms still fuses everything behind
 * them: a host-evaluated reward column (GF_R_EXTERNAL) has to be computed after the termination phase and before the reward
 * phase (managed_env.py:303-319: the callable may read this step's termination buffers), so the step is
 * termination launch -> the callables -> ONE launch for reward ... observation.  Any termination table is then acceptable,
 * including GF_T_EXTERNAL terms.
 * GF_POST_OBSERVE_ONLY: every phase of the step up to and including the reset has ALREADY run — the termination phase, the
 * rewards, the command managers and the reset of the done envs (gf_masked_reset on `reset`, by mask or by the index list a user's
 * `reset(envs_idx)` override took: managed_env.py:308-310) — and only the observation managers are left (managed_env.py:324).
 * The launch reads `terminated` / `truncated` (an env reset in this tick is observed through `reset->quat_stash`, the stale-cache
 * quirk of entity_manager.py:189-195) and runs the observation waves of the fused kernel for up to two managers as one launch;
 * `reward`, the command and gait lists must be empty.  This is the observation part of a step whose reset goes through user
 * code.
 * GF_POST_NO_RESET: the counterpart for the FRONT of such a step — termination, rewards, command.step / gait.step as one launch,
 * and nothing after them: no env is reset (the masks are written; the reset follows by index list through user code, then the
 * observation-only launch), `reset`, `command_reset[]`, `gait_reset[]` may be NULL, `num_observe` must be 0. */
enum { GF_POST_TERMINATION_DONE = 1, GF_POST_OBSERVE_ONLY = 2, GF_POST_NO_RESET = 4 };
typedef struct GfPostRefs {
    const GfTerminationArgs* termination;                 /* required */
    const GfRewardArgs* reward;                           /* may be NULL */
    const GfResetArgs* reset;                             /* required; mask/mask2 must be termination's outputs */
    int32_t num_command;
    int32_t num_observe;
    const GfCommandArgs* command_step[GF_POST_MAX_CMD];   /* mode GF_CMD_STEP  */
    const GfCommandArgs* command_reset[GF_POST_MAX_CMD];  /* mode GF_CMD_MASKED on the same masks, same buffers */
    const GfObservationArgs* observe[GF_POST_MAX_OBS];
    /* GaitCommandManagers stepped / reset inside the same launch (examples/gait_trainer: BASELINE config 5).  The swing / stance
     * bytes (GfGaitArgs.wave_flags) are read ACROSS 64-env blocks by GF_R_GAIT_PHASE (env-0 quirk) while every block rewrites its
     * own byte, so a single launch needs two buffers: it reads gait_step->wave_flags (the state the previous step left; must be
     * the reward descriptor's gait_wave_flags) and writes every block's byte for the state it leaves into gait_flags_next, which
     * the caller makes the current buffer afterwards (ping-pong).  Sequentially the result is the same: gait.step rewrites every
     * block's byte, gait.reset the blocks with a reset env, both from the rows they hold. */
    int32_t num_gait;
    int32_t flags;                                    /* GF_POST_* bits */
    const GfGaitArgs* gait_step[GF_POST_MAX_GAIT];    /* mode GF_CMD_STEP */
    const GfGaitArgs* gait_reset[GF_POST_MAX_GAIT];   /* mode GF_CMD_MASKED on the termination masks, same state */
    uint8_t* gait_flags_next[GF_POST_MAX_GAIT];       /* same size as wave_flags; may be NULL when wave_flags is NULL */
    /* optional: the launch also stores the step's observation / reward / done flags into rollout-storage rows (§8f-5).
     * rollout->obs must be the obs buffer of one of `observe`, ->reward the reward buffer, the masks termination's outputs. */
    const GfRolloutArgs* rollout;
} GfPostRefs;

int gf_post_physics_check(const GfPostRefs* r);               /* GF_OK if gf_post_physics_step can fuse this combination */
int gf_post_physics_step(const GfPostRefs* r, void* stream);  /* replaces managed_env.py:303-326 in one launch */
/* The same launch with the scene's ContactManagers stepped IN FRONT of the other phases (SURVEY.md §8f-1 ∘ §8f-2): the reference runs
 * contact.step, termination, reward … back to back per env (managed_env.py:294-326, managers/contact/contact_manager.py:384-477,
 * managers/contact/kernel.py:35-90), and the fused launch works on the same 64-env tiles and reads what the contact step just
 * wrote — so `contacts[0 .. num_contacts)` (up to four GfContactArgs over the same scene arrays: what gf_contact_step takes, one
 * per manager) run as the first phase of the launch: slot ids staged in the tile's LDS, one lane per (env, tracked link), the
 * managers' public buffers written as gf_contact_step writes them, a workgroup barrier, then termination … observation.  By
 * construction the results are those of gf_contact_step per manager followed by gf_post_physics_step.  GF_E_UNSUPPORTED when the
 * managers cannot be folded (more than 32 tracked links or 16 with-filter links, link ids above 254, slot rows beyond the tile's
 * LDS, a statistics block other than the step's, GF_POST_OBSERVE_ONLY): the caller runs gf_contact_step itself. */
int gf_post_physics_step_contacts(const GfPostRefs* r, const GfContactArgs* const* contacts, int num_contacts, void* stream);
/* Writes "program <id> (<name>): <structure signature>" for this combination into buf: which kernel
 * gf_post_physics_step would launch (id 0 = table interpreter, >0 = a static program compiled for exactly this
 * structure) and the signature in the notation of csrc/gf_post_programs.h.  Host-only, no GPU needed. */
int gf_post_physics_describe(const GfPostRefs* r, char* buf, int cap);
/* The dynamic LDS, in bytes, the fused launch of this combination asks for (the program gf_post_physics_describe names; tick != 0:
 * its variant with the scene tick as prologue, where it has one; without a folded contact phase), and the same for the table
 * interpreter of a DOF count at a single-frame observation width, which bounds every admitted descriptor.  Host-only, no GPU needed. */
int gf_post_physics_lds_bytes(const GfPostRefs* r, int tick, long* bytes_out);
long gf_post_interp_lds_bytes(int num_dofs, int obs_width, int num_gait, int tick);
/* Which state arrays the fused launch of this combination reads, as packed: a word of GF_POST_NEEDS_* bits.  An array whose bit is
 * off is never read — a role that would take its rows sees zeros.  Host-only, no GPU needed. */
enum { GF_POST_NEEDS_POS = 1, GF_POST_NEEDS_QUAT = 2, GF_POST_NEEDS_LIN = 4, GF_POST_NEEDS_ANG = 8, GF_POST_NEEDS_DOFPOS = 16,
       GF_POST_NEEDS_DOFVEL = 32, GF_POST_NEEDS_TARGETS = 64, GF_POST_NEEDS_ACTIONS = 128, GF_POST_NEEDS_LAST = 256,
       GF_POST_NEEDS_EPLEN = 512, GF_POST_NEEDS_MAXLEN = 1024, GF_POST_NEEDS_DOFDEV = 2048 /* the reward wave's dof_pos rows */,
       GF_POST_NEEDS_ACTRATE = 4096 /* the reward wave's action / last-action rows */, GF_POST_NEEDS_DOFFORCE = 8192 };
int gf_post_physics_needs(const GfPostRefs* r, uint32_t* needs_out);
/* Static programs for configs the library was not built with.  The reference's configs are live Python dicts
 * (managers/config/config_item.py:31-44; reward_manager.py:166-195 walks whatever the dict holds), so a user's task is not
 * one of the compiled-in structures; it would run the table interpreter (about 1.3 x the kernel time).  Instead the host
 * generates the program struct of the recorded step's signature (gf_post_physics_describe), compiles csrc/gf_post_ws.h with it
 * for gfx950 into a small shared object (hipcc, a few seconds, cached by signature; genesis_forge_amd/_programs.py) and
 * registers it here: from then on gf_post_physics_step launches the plugin's post_ws_kernel<Program> for every descriptor
 * that matches it — ids from 100 upwards in gf_post_physics_describe.  Structure only: weights, parameters, ranges, scales
 * stay run-time kernel arguments, a config whose STRUCTURE changes simply stops matching (interpreter until its own program is
 * there).  The plugin exports gfp_abi_version / gfp_args_size (checked against this library: GF_E_UNSUPPORTED on a mismatch or
 * an unloadable file) / gfp_name / gfp_matches / gfp_kernel / gfp_lds_bytes.  Append-only, at most 256, thread-safe. */
int gf_post_program_register(const char* plugin_path, int* program_id_out);
int gf_post_program_count(void);

/* ------------------------------------------------------------------------------------------
 * Recorded step: the fixed launch sequence of one ManagedEnvironment.step() replayed with a single
 * call.  The host records the (phase, descriptor) pairs of one ordinary step, keeps the descriptors
 * alive, patches the few per-step fields (action pointer, RNG stream ids, observation ring slots) in
 * place and replays — the phase order of managed_env.py:274-334 without per-launch host work.
 * ---------------------------------------------------------------------------------------- */
typedef struct GfOp {
    int32_t phase;      /* GF_PHASE_* or GF_OP_* */
    int32_t _pad;
    const void* args;   /* the phase's descriptor (GfActionArgs*, …) */
} GfOp;

enum { GF_OP_STATS_CLEAR = 100, GF_OP_STATS_COPY = 101, GF_OP_POST_PHYSICS = 102 /* args = GfPostRefs* */,
       GF_OP_STATS_PACK = 103 /* args = GfStatsPackArgs* */ };

/* Fold the GF_STATS_SHARDS shards of one statistics block into the f64 vector that is all-reduced across ranks
 * (layout: term_fired[GF_MAX_TERM_TERMS], reset_count, nan_flag, inf_flag, contact_flag, resample_count,
 * reward_episode_sum[GF_MAX_TERMS], gait_count[GF_MAX_GAITS]; flags fold with max, everything else adds). */
#define GF_STATS_VECTOR_LEN (GF_MAX_TERM_TERMS + 5 + GF_MAX_TERMS + GF_MAX_GAITS)
typedef struct GfStatsPackArgs {
    const GfStepStats* src;   /* device, GF_STATS_SHARDS blocks */
    double* dst;              /* device, GF_STATS_VECTOR_LEN */
} GfStatsPackArgs;
int gf_stats_pack(const GfStatsPackArgs* a, void* stream);

/* rows: [num_rows <= 64][GF_STATS_VECTOR_LEN] consecutive packed (and, with a process group, all-reduced) statistics rows, oldest
 * first.  Copies the NEWEST row whose reset_count entry is > 0 to dst; leaves dst alone when no row reset anything.  This keeps
 * "the episode means of the last reset" (reward_manager.py:138-153, :197-222 — the reference refreshes them inside every reset())
 * on the device when ring rows are recycled unread, so the host never has to read a row just to carry that value forward. */
int gf_stats_last_reset(const double* rows, int num_rows, double* dst, void* stream);

typedef struct GfStatsCopyArgs {
    const GfStepStats* src;   /* device, GF_STATS_SHARDS blocks */
    void* dst;                /* pinned host, GF_STATS_SHARDS * sizeof(GfStepStats) */
    void* event;              /* from gf_event_create(); recorded after the copy; may be NULL */
} GfStatsCopyArgs;

/* Runs the ops in order; stops at the first op that fails and reports its index.  Neighbouring ops share launches where that gives
 * the same results: an action op directly in front of a stand-in scene op runs inside the tick's launch (GF_FOLD_ACTION=0: not), and
 * with a GF_OP_POST_PHYSICS op directly behind that pair — a recorded step on the stand-in scene without per-link rows or contact
 * slots — the three ops are ONE launch, the tick as the post-physics kernel's prologue (GF_FOLD_STEP=0: not; both switches are
 * read per call); contact ops in front of a post-physics op are its first phase (GF_OPT_FOLD_CONTACT); runs of per-env phases chain
 * (GF_OPT_CHAIN).  A profiled phase keeps its own launch.  Return codes and failed_index do not depend on any of this. */
int gf_run_ops(const GfOp* ops, int num_ops, void* stream, int* failed_index);
/* steps gf_run_ops ran as one launch since the library was loaded */
long gf_step_fold_count(void);

/* Recorded step, patched natively: the few descriptor fields that change from one step to the next are described ONCE as a
 * patch table (which host address receives what), and a step is a single call — apply the table, then gf_run_ops — instead of
 * a Python closure per phase (managed_env.py:274-334 has no counterpart: the reference re-marshals every op every step).
 * All state lives in caller-owned memory (the descriptors, the counters and rotors the table points at): the call itself is
 * stateless and re-entrant per recorded step. */
enum {
    GF_PATCH_ACTIONS = 1,    /* *(const void**)target = actions                                    (the policy output of this step) */
    GF_PATCH_STREAM = 2,     /* *(uint64_t*)target = ++*rng_stream                                 (Philox stream ids, in draw order) */
    GF_PATCH_COUNTER = 3,    /* *(uint64_t*)target = (*(uint64_t*)aux)++                           (scene tick) */
    GF_PATCH_ROTATE = 4,     /* r = (GfRotor*)aux: if target: *(void**)target = r->slot[r->cur]; r->cur = (r->cur + 1) % r->count;
                                if target2: *(void**)target2 = r->slot[r->cur]                     (output slots, ping-pong buffers) */
    GF_PATCH_PARAM = 5,      /* *(const void**)target = params[index]                              (statistics ring slots) */
    GF_PATCH_COPY = 6,       /* *(uint64_t*)target = *(const uint64_t*)aux                         (a field that follows another) */
    GF_PATCH_RING_SLOT = 7,  /* c = (GfRingClock*)aux: *(int32_t*)target = (c->length - c->calls % c->length) % c->length + 1; ++c->calls;
                                if target2: *(int32_t*)target2 = the same value
                                                              (GfObservationArgs.history_ring, GfHistoryUnrollArgs.ring_slot) */
    GF_PATCH_PARAM_OFFSET = 8 /* *(const char**)target = (const char*)params[index] + (intptr_t)aux
                                 (a scene with Genesis' public surface only: every getter — entity.get_pos() …,
                                 collider.get_contacts(), rigid_solver.get_links_quat(); entity_manager.py:189-195,
                                 contact_manager.py:384-400 — returns a NEW tensor each tick; params[index] is this tick's tensor,
                                 aux the byte offset of the field's view inside it.  A NULL params[index] is refused: GF_E_NULL) */
};
typedef struct GfRotor {
    int32_t cur;
    int32_t count;           /* 1..8 */
    void* slot[8];
} GfRotor;
typedef struct GfRingClock {
    int32_t calls;
    int32_t length;
} GfRingClock;
typedef struct GfReplayPatch {
    int32_t kind;            /* GF_PATCH_* */
    int32_t index;           /* GF_PATCH_PARAM */
    void* target;
    void* target2;
    void* aux;
} GfReplayPatch;
typedef struct GfReplay {
    const GfOp* ops;         /* may be NULL / num_ops 0: patch only (the caller then replays the ops in pieces) */
    int32_t num_ops;
    int32_t num_patches;
    const GfReplayPatch* patches;
    uint64_t* rng_stream;    /* the env's stream counter (GF_PATCH_STREAM pre-increments it) */
} GfReplay;
int gf_replay_step(const GfReplay* r, const void* actions, const void* const* params, int num_params, void* stream, int* failed_index);
/* The same replay as ONE hipGraphLaunch: the first call builds a linear hipGraph of the step's kernel launches, later calls
 * refresh every node's kernel arguments in place (the descriptors change from step to step: action pointer, RNG streams,
 * ring slots) and launch the graph — the host pays one graph launch instead of one launch per kernel.  *cache is an opaque
 * handle (start with NULL, release with gf_graph_destroy).  Falls back to gf_run_ops when the step contains memset / copy
 * ops, a phase is being profiled, GF_OPT_GRAPH is 0 or the graph API refuses. */
int gf_run_ops_graph(void** cache, const GfOp* ops, int num_ops, void* stream, int* failed_index);
int gf_graph_destroy(void** cache);
void* gf_event_create(void);
int gf_event_destroy(void* event);
int gf_event_synchronize(void* event);   /* blocks the host until the event has completed */

/* Optional per-phase HIP-event timing used by bench.py (events recorded on `stream`
 * immediately around the kernel launch of the selected phase). */
enum { GF_PHASE_ACTION = 0, GF_PHASE_CONTACT, GF_PHASE_TERMINATION, GF_PHASE_REWARD, GF_PHASE_COMMAND,
       GF_PHASE_RESET, GF_PHASE_OBSERVE, GF_PHASE_ROTATE, GF_PHASE_SCENE, GF_PHASE_POST, GF_PHASE_TERRAIN, GF_PHASE_GAIT, GF_PHASE_ROLLOUT,
       GF_PHASE_UNROLL, GF_PHASE_ROLLOUT_POLICY, GF_PHASE_GAE, GF_PHASE_COMPACT, GF_PHASE_COUNT };
int gf_profile_begin(int phase, int max_samples);     /* start recording event pairs for `phase` */
int gf_profile_end(double* total_ms, int* samples);    /* sync events, return Σ elapsed + count, free them */

#ifdef __cplusplus
}
#endif
#endif /* GF_STEP_H */
