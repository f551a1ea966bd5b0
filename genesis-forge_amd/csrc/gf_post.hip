// gf_post.hip — host side of the fused post-physics step: termination → reward → command.step → reset of done envs →
// command.reset → observations (managed_env.py:303-326) as ONE launch.  The kernel itself is post_ws_kernel<P> (gf_post_ws.h);
// this file decides whether a step can run on it, describes the step to it and picks the program it runs.
//   * pack() checks that the per-phase descriptors of a GfPostRefs describe one fusable step — the same env count, seed and
//     masks in every phase, buffers that alias only where the kernel expects them to, sizes inside the kernel's tables — and
//     packs them into one GfPostArgs (gf_post_args.h): shared views deduplicated, term / item slots remapped onto them, the
//     `needs` bits that say which per-env inputs the launch loads.  Anything else is GF_E_UNSUPPORTED and the caller runs the
//     phases one by one (GF_POST_WHY=1 names the rule).
//   * fold_contacts() adds the scene's ContactManagers as a phase in front of the others (GfPostArgs.cfold), or refuses and
//     leaves the contact kernel a launch of its own.
//   * the program table: one PostProgram record per program — name, matcher, kernel handle, LDS size, whether it carries the contact
//     phase, its tick variant — for the static programs of gf_post_programs.h (kBuiltin), the table interpreter Interp<DV, TAIL> by DOF
//     count (kInterp) and the programs compiled at run time and registered through gf_post_program_register (g_dyn); select_program()
//     matches a packed descriptor against them once per step.
//   * post_launch() sizes the LDS for the selected record and launches its kernel by handle.
// Semantics are, by construction, those of calling the phase entry points in sequence (the oracle twin does exactly that);
// tests compare the two paths bit for bit.
// Algorithmic traffic, Go2 command config: R 13·4 + 5 rows·48 + cmd 12 + ep/max 8 + secs 4 + sums 24 = 340,
// W masks 2 + reward 4 + sums 24 + secs 4 + obs 192 = 226  →  566 B/env.
#include <dlfcn.h>

#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <mutex>

#include "gf_post_args.h"
#include "gf_post_ws.h"
#include "gf_post_programs.h"

namespace gf {

// ------------------------------------------------------------------------------------------------------------
// pack(): validate that the per-phase descriptors describe one fusable step and pack them.
// ------------------------------------------------------------------------------------------------------------
static int cmd_slot_of_reward_op(int op) {
    switch (op) {
        case GF_R_CMD_TRACK_LIN_VEL:
        case GF_R_CMD_TRACK_ANG_VEL:
        case GF_R_STAND_STILL: return 0;
        case GF_R_FEET_AIR_TIME: return 1;
        default: return -1;
    }
}
static bool reward_op_has_contact(int op) { return op == GF_R_HAS_CONTACT || op == GF_R_CONTACT_FORCE || op == GF_R_FEET_AIR_TIME || op == GF_R_FEET_SLIDE; }
static bool term_op_has_contact(int op) { return op == GF_T_HAS_CONTACT || op == GF_T_CONTACT_FORCE || op == GF_T_CONTACT_FORCE_GRACE; }

struct Packer {
    GfPostArgs a{};
    int n_contact = 0, n_view = 0;

    int contact_slot(const GfContactView& v) {
        for (int k = 0; k < n_contact; ++k)
            if (a.contact[k].contacts == v.contacts) {
                if (!a.contact[k].link_vel) a.contact[k].link_vel = v.link_vel;
                if (!a.contact[k].link_pos) a.contact[k].link_pos = v.link_pos;
                return k;
            }
        if (n_contact >= GF_MAX_CONTACT_VIEWS) return -1;
        a.contact[n_contact] = v;
        return n_contact++;
    }
    int view_slot(const GfCommandView& v) {
        for (int k = 0; k < n_view; ++k)
            if (a.command[k].command == v.command && a.command[k].width == v.width && a.command[k].stride == v.stride) return k;
        if (n_view >= GF_MAX_COMMAND_VIEWS) return -1;
        a.command[n_view] = v;
        a.cmd_of_view[n_view] = -1;
        if (a.n_gait && v.command == a.gait.state) {
            // a view of the gait manager's state rows (observation(): 14 columns of the 16-float row): travels through LDS
            if (v.stride != GF_GAIT_ROW || v.width > GF_GAIT_ROW) return -1;
            a.cmd_of_view[n_view] = kViewGait;
            return n_view++;
        }
        for (int c = 0; c < a.n_cmd; ++c)
            if (a.cmds[c].command == v.command) {
                // a fused command manager's own buffer is dense and travels through registers / LDS: a strided alias of it
                // (a column view of a resampled command) stays on the phase-by-phase path
                if (v.stride && v.stride != v.width) return -1;
                a.cmd_of_view[n_view] = c;
            }
        return n_view++;
    }
};

static bool same_entity(const GfEntityView& x, const GfEntityView& y) {
    auto ok = [](const float* p, const float* q) { return !p || !q || p == q; };
    return ok(x.pos, y.pos) && ok(x.quat, y.quat) && ok(x.lin_vel, y.lin_vel) && ok(x.ang_vel, y.ang_vel);
}
static void merge_entity(GfPostArgs& a, const GfEntityView& v) {
    if (v.pos) a.pos = const_cast<float*>(v.pos);
    if (v.quat) a.quat = const_cast<float*>(v.quat);
    if (v.lin_vel) a.lin_vel = const_cast<float*>(v.lin_vel);
    if (v.ang_vel) a.ang_vel = const_cast<float*>(v.ang_vel);
}

// GF_POST_WHY=1 in the environment names the rule that kept a step from fusing (development aid; checked once)
static bool why_enabled() {
    static const bool on = getenv("GF_POST_WHY") != nullptr;
    return on;
}
#define UNSUP(cond)                                                                                  \
    do {                                                                                             \
        if (cond) {                                                                                  \
            if (why_enabled()) fprintf(stderr, "gf_post_physics: not fusable (%s:%d): %s\n", __FILE__, __LINE__, #cond); \
            return GF_E_UNSUPPORTED;                                                                 \
        }                                                                                            \
    } while (0)

static int pack(const GfPostRefs* r, Packer& pk) {
    if (!r || !r->termination) return GF_E_NULL;
    // GF_POST_NO_RESET: termination … command / gait step, nothing behind them.  There is no reset to describe, so `reset` and the
    // masked command / gait descriptors may be absent; the checks below then run against a stand-in that says "no section of the
    // reset applies" (the seed / env offset every phase shares comes from the first stepped manager).
    const bool no_reset = (r->flags & GF_POST_NO_RESET) != 0;
    if (!no_reset && !r->reset) return GF_E_NULL;
    GfPostArgs& a = pk.a;
    const GfTerminationArgs& T = *r->termination;
    GfResetArgs none{};
    if (no_reset && !r->reset) {
        none.num_envs = T.num_envs; none.mask = T.terminated; none.mask2 = T.truncated;
        none.num_dofs = r->reward ? r->reward->num_dofs : 0;
        if (r->num_command > 0 && r->command_step[0]) { none.seed = r->command_step[0]->seed; none.env_offset = r->command_step[0]->env_offset; }
        else if (r->num_gait > 0 && r->gait_step[0]) { none.seed = r->gait_step[0]->seed; none.env_offset = r->gait_step[0]->env_offset; }
    }
    const GfResetArgs& RS = r->reset ? *r->reset : none;
    const GfRewardArgs* RW = r->reward;
    const int N = T.num_envs;
    UNSUP(no_reset && (r->num_observe != 0 || r->rollout || (r->flags & GF_POST_OBSERVE_ONLY)));
    a.no_reset = no_reset ? 1 : 0;
    // GF_POST_OBSERVE_ONLY: the step's phases up to the reset have run as launches of their own; `reset` is the descriptor that reset
    // ran with (its masks, its stale-quaternion stash, the seed every phase shares) and nothing in it is applied again
    const bool obs_only = (r->flags & GF_POST_OBSERVE_ONLY) != 0;
    UNSUP(obs_only && (r->reward || r->num_command || r->num_gait || r->rollout || r->num_observe < 1));
    a.obs_only = obs_only ? 1 : 0;
    UNSUP(N <= 0 || T.num_terms > kPostMaxTerm || T.term_out);
    UNSUP(r->num_command < 0 || r->num_command > GF_POST_MAX_CMD || r->num_observe < 0 || r->num_observe > GF_POST_MAX_OBS);
    UNSUP(RS.num_envs != N || RS.mask != T.terminated || RS.mask2 != T.truncated);
    UNSUP(RS.len_draws || RS.dof_draws);
    bool have_terrain = false;  // one terrain map per fused step: the reward's and the spawn's must be the same
    a.num_envs = N;
    a.terminated = T.terminated; a.truncated = T.truncated;
    a.stats = obs_only ? nullptr : (T.stats ? T.stats : RS.stats);   // (an observation-only launch counts nothing)
    UNSUP(!obs_only && RS.stats && T.stats && RS.stats != T.stats);
    a.episode_length = const_cast<int32_t*>(T.episode_length);
    a.max_episode_length = const_cast<int32_t*>(T.max_episode_length);
    a.has_maxlen = T.max_episode_length != nullptr;
    merge_entity(a, T.entity);
    uint32_t needs = 0;
    int D = RS.num_dofs;

    // commands first (views map onto them)
    a.n_cmd = r->num_command;
    for (int c = 0; c < a.n_cmd; ++c) {
        const GfCommandArgs* s = r->command_step[c];
        const GfCommandArgs* m = r->command_reset[c];
        UNSUP(!s || (!m && !no_reset) || s->mode != GF_CMD_STEP);
        UNSUP(s->num_envs != N || s->num_ranges > kPostMaxRanges || s->draws || s->resample_steps <= 0 || s->episode_length != T.episode_length);
        UNSUP(s->seed != RS.seed || s->env_offset != RS.env_offset);
        if (m) {
            UNSUP(m->mode != GF_CMD_MASKED || s->command != m->command || s->num_ranges != m->num_ranges || m->num_envs != N || m->draws);
            UNSUP(m->mask != T.terminated || m->mask2 != T.truncated || m->seed != RS.seed || m->env_offset != RS.env_offset);
        }
        UNSUP(s->stats && a.stats && s->stats != a.stats);
        PostCmd& pc = a.cmds[c];
        pc.command = s->command; pc.width = s->num_ranges; pc.resample_steps = s->resample_steps;
        pc.stream_step = s->stream; pc.stream_reset = m ? m->stream : 0;
        for (int j = 0; j < s->num_ranges; ++j) {
            UNSUP(m && (s->lo[j] != m->lo[j] || s->hi[j] != m->hi[j]));
            pc.lo[j] = s->lo[j]; pc.hi[j] = s->hi[j];
        }
        needs |= PN_EPLEN;
    }
    a.seed = RS.seed; a.env_offset = RS.env_offset; a.stream_reset = RS.stream;

    // the GaitCommandManager (examples/gait_trainer): stepped and reset on wave 0's registers
    UNSUP(r->num_gait < 0 || r->num_gait > GF_POST_MAX_GAIT);
    a.n_gait = r->num_gait;
    if (a.n_gait) {
        const GfGaitArgs* gs = r->gait_step[0];
        const GfGaitArgs* gm = r->gait_reset[0];
        UNSUP(!gs || (!gm && !no_reset) || gs->mode != GF_CMD_STEP || !gs->state || !gs->selected);
        UNSUP(gs->num_envs != N || gs->draws || gs->resample_steps <= 0 || gs->num_gaits < 1 || gs->num_gaits > GF_MAX_GAITS || gs->episode_length != T.episode_length);
        UNSUP(gs->seed != RS.seed || gs->env_offset != RS.env_offset);
        UNSUP(gs->stats && a.stats && gs->stats != a.stats);
        UNSUP((gs->wave_flags != nullptr) != (r->gait_flags_next[0] != nullptr) || (gs->wave_flags && gs->wave_flags == r->gait_flags_next[0]));
        UNSUP(reinterpret_cast<uintptr_t>(gs->state) & 15u);
        if (gm) {
            UNSUP(gm->mode != GF_CMD_MASKED || gs->state != gm->state || gs->selected != gm->selected || gm->num_envs != N || gm->draws);
            UNSUP(gm->mask != T.terminated || gm->mask2 != T.truncated || gm->seed != RS.seed || gm->env_offset != RS.env_offset);
            UNSUP(gs->wave_flags != gm->wave_flags);
            // both descriptors are filled from the same manager state (curriculum values are re-read per launch)
            UNSUP(gs->num_gaits != gm->num_gaits || gs->fixed_clearance_mask != gm->fixed_clearance_mask || gs->dt != gm->dt || gs->two_pi != gm->two_pi);
            UNSUP(memcmp(gs->cum_weight, gm->cum_weight, sizeof(gs->cum_weight)) != 0 || memcmp(gs->gait_offsets, gm->gait_offsets, sizeof(gs->gait_offsets)) != 0);
            UNSUP(gs->clearance_lo != gm->clearance_lo || gs->clearance_hi != gm->clearance_hi || gs->period_lo != gm->period_lo || gs->period_hi != gm->period_hi);
        }
        PostGait& pg = a.gait;
        pg.state = gs->state; pg.selected = gs->selected; pg.flags_in = gs->wave_flags; pg.flags_out = r->gait_flags_next[0];
        pg.stream_step = gs->stream; pg.stream_reset = gm ? gm->stream : 0;
        pg.resample_steps = gs->resample_steps; pg.num_gaits = gs->num_gaits; pg.fixed_clearance_mask = gs->fixed_clearance_mask;
        memcpy(pg.cum_weight, gs->cum_weight, sizeof(pg.cum_weight));
        memcpy(pg.gait_offsets, gs->gait_offsets, sizeof(pg.gait_offsets));
        pg.clearance_lo = gs->clearance_lo; pg.clearance_hi = gs->clearance_hi; pg.period_lo = gs->period_lo; pg.period_hi = gs->period_hi;
        pg.dt = gs->dt; pg.two_pi = gs->two_pi;
        needs |= PN_EPLEN;
    }

    // termination terms (not evaluated when the phase has already run as a launch of its own: the masks are inputs then)
    a.term_done = ((r->flags & GF_POST_TERMINATION_DONE) || obs_only) ? 1 : 0;
    a.num_term = a.term_done ? 0 : T.num_terms;
    for (int k = 0; k < a.num_term; ++k) {
        GfTerm t = T.terms[k];
        switch (t.op) {
            case GF_T_TIMEOUT: if (T.max_episode_length) needs |= PN_EPLEN | PN_MAXLEN; break;
            case GF_T_BAD_ORIENTATION: needs |= PN_QUAT | PN_EPLEN; break;
            case GF_T_BASE_HEIGHT_BELOW:
            case GF_T_OUT_OF_BOUNDS: needs |= PN_POS; break;
            case GF_T_CONTACT_FORCE_GRACE: needs |= PN_EPLEN;  // fallthrough
            case GF_T_HAS_CONTACT:
            case GF_T_CONTACT_FORCE: break;
            default: return GF_E_UNSUPPORTED;  // GF_T_EXTERNAL: a host-evaluated column needs GF_POST_TERMINATION_DONE (the table is then not evaluated here)
        }
        if (term_op_has_contact(t.op)) {
            UNSUP(t.i[0] < 0 || t.i[0] >= GF_MAX_CONTACT_VIEWS || !T.contact[t.i[0]].contacts);
            const int s = pk.contact_slot(T.contact[t.i[0]]);
            UNSUP(s < 0);
            t.i[0] = s;
        }
        a.tterms[k] = t;
    }

    // reward
    a.num_rew = -1;
    if (RW) {
        UNSUP(RW->num_envs != N || RW->mode != GF_REWARD_MODE_STEP || RW->num_terms > kPostMaxReward || !RW->reward || !RW->episode_seconds);
        UNSUP(!same_entity(T.entity, RW->entity));
        merge_entity(a, RW->entity);
        a.num_rew = RW->num_terms;
        a.reward = RW->reward; a.episode_sums = RW->episode_sums; a.episode_seconds = RW->episode_seconds;
        a.logging = RW->logging_enabled && RW->episode_sums;
        a.dt = RW->dt;
        for (int s = 0; s < 4; ++s) a.state[s] = RW->state[s];
        // view 0 first so the kernel's preloaded cmd0 refers to it
        if (RW->command[0].command) UNSUP(pk.view_slot(RW->command[0]) != 0);
        uint32_t covered = 0;
        for (int k = 0; k < RW->num_terms; ++k) {
            GfTerm t = RW->terms[k];
            UNSUP(t.row < 0 || t.row >= 24);
            covered |= 1u << t.row;
            switch (t.op) {
                case GF_R_IS_ALIVE:
                case GF_R_TERMINATED: UNSUP(RW->terminated != T.terminated); break;
                case GF_R_BASE_HEIGHT:
                    needs |= PN_POS;
                    if (t.flags & GF_RW_FLAG_TERRAIN) {
                        UNSUP(RW->terrain.height_field && (RW->terrain.rows < 1 || RW->terrain.cols < 1));
                        UNSUP(have_terrain && memcmp(&a.terrain, &RW->terrain, sizeof(GfTerrainView)) != 0);
                        a.terrain = RW->terrain;
                        have_terrain = true;
                    }
                    break;
                case GF_R_DOF_SIMILAR_TO_DEFAULT:
                case GF_R_STAND_STILL: needs |= PN_DOFPOS | PN_DOFDEV; break;
                case GF_R_LIN_VEL_Z_L2: needs |= PN_QUAT | PN_LIN; break;
                case GF_R_ANG_VEL_XY_L2: needs |= PN_QUAT | PN_ANG; break;
                case GF_R_FLAT_ORIENTATION_L2: needs |= PN_QUAT; break;
                case GF_R_BODY_ACCEL_EXP: needs |= PN_QUAT | PN_LIN | PN_ANG; UNSUP(t.i[0] < 0 || t.i[0] >= 4 || !RW->state[t.i[0]]); break;
                case GF_R_ACTION_RATE_L2: needs |= PN_ACTIONS | PN_LAST | PN_ACTRATE; break;
                case GF_R_CMD_TRACK_LIN_VEL: needs |= PN_QUAT | PN_LIN; break;
                case GF_R_CMD_TRACK_ANG_VEL: needs |= PN_QUAT | PN_ANG; break;
                case GF_R_HAS_CONTACT:
                case GF_R_CONTACT_FORCE:
                case GF_R_FEET_AIR_TIME:
                case GF_R_FEET_SLIDE: break;
                case GF_R_GAIT_PHASE:
                case GF_R_FOOT_HEIGHT: {
                    // read the feet's contact / velocity / position buffers and the PRE-step gait rows straight from memory
                    UNSUP(t.i[0] < 0 || t.i[0] >= GF_MAX_CONTACT_VIEWS || !RW->contact[t.i[0]].contacts || !RW->contact[t.i[0]].link_vel);
                    UNSUP(t.op == GF_R_FOOT_HEIGHT && !RW->contact[t.i[0]].link_pos);
                    UNSUP(t.i[1] < 0 || t.i[1] >= GF_MAX_COMMAND_VIEWS || !RW->command[t.i[1]].command || RW->command[t.i[1]].stride != GF_GAIT_ROW);
                    for (int f = 0; f < 4; ++f) UNSUP(((t.i[2] >> (8 * f)) & 0xff) >= RW->contact[t.i[0]].num_links);
                    const int cs2 = pk.contact_slot(RW->contact[t.i[0]]);
                    const int vs2 = pk.view_slot(RW->command[t.i[1]]);
                    UNSUP(cs2 < 0 || vs2 < 0);
                    t.i[0] = cs2; t.i[1] = vs2;
                    if (t.op == GF_R_GAIT_PHASE && RW->gait_wave_flags) {
                        UNSUP(!a.n_gait || RW->gait_wave_flags != a.gait.flags_in);   // the bytes this launch may read are the ones it does not write
                        a.gait_wave_flags = RW->gait_wave_flags;
                    }
                } break;
                case GF_R_EXTERNAL:   // a column the host evaluated after the termination phase: only behind GF_POST_TERMINATION_DONE
                    UNSUP(!a.term_done || t.i[0] < 0 || t.i[0] >= GF_MAX_EXT || !RW->ext[t.i[0]]);
                    a.ext[t.i[0]] = RW->ext[t.i[0]];
                    break;
                default: return GF_E_UNSUPPORTED;
            }
            if (t.op == GF_R_BASE_HEIGHT && (t.flags & GF_RW_FLAG_CMD)) {
                UNSUP(t.i[0] < 0 || t.i[0] >= GF_MAX_COMMAND_VIEWS || !RW->command[t.i[0]].command);
                const int s = pk.view_slot(RW->command[t.i[0]]);
                UNSUP(s < 0 || pk.a.cmd_of_view[s] >= 0);  // a resampled buffer as height target: keep the unfused path
                t.i[0] = s;
            }
            const int cs = cmd_slot_of_reward_op(t.op);
            if (cs >= 0 && t.i[cs] >= 0) {
                UNSUP(t.i[cs] >= GF_MAX_COMMAND_VIEWS || !RW->command[t.i[cs]].command);
                const int s = pk.view_slot(RW->command[t.i[cs]]);
                UNSUP(s < 0);
                // terms read view 0 from registers and any other view from memory — as it is BEFORE this step's resample: every
                // command / gait row the launch rewrites is stored behind the barrier the reward wave passes after its fold
                t.i[cs] = s;
            }
            if (reward_op_has_contact(t.op)) {
                UNSUP(t.i[0] < 0 || t.i[0] >= GF_MAX_CONTACT_VIEWS || !RW->contact[t.i[0]].contacts);
                const int s = pk.contact_slot(RW->contact[t.i[0]]);
                UNSUP(s < 0);
                t.i[0] = s;
            }
            a.rterms[k] = t;
        }
        if (needs & (PN_DOFPOS | PN_DOFDEV)) {
            UNSUP(!RW->dof_pos || !RW->default_dof_pos);
            a.dof_pos = const_cast<float*>(RW->dof_pos);
            a.default_dof_pos = RW->default_dof_pos;
            D = RW->num_dofs;
        }
        if (needs & PN_ACTIONS) {
            UNSUP(!RW->actions || !RW->last_actions);
            a.env_actions = const_cast<float*>(RW->actions);
            a.env_last_actions = const_cast<float*>(RW->last_actions);
            D = RW->num_dofs;
        }
        // reward-manager reset section must address the same buffers
        UNSUP(RS.episode_seconds && RS.episode_seconds != RW->episode_seconds);
        UNSUP(RS.episode_sums && RS.episode_sums != RW->episode_sums);
        UNSUP(!no_reset && !RS.episode_seconds);  // the fused kernel always resets the seconds of done envs
        UNSUP(!no_reset && (RS.reward_logging != 0) != (a.logging != 0));
        a.reward_rows = RS.num_reward_terms;
        a.reward_log_mask = RS.reward_log_mask;
        a.uncovered_rows = 0;
        for (int row = 0; row < RS.num_reward_terms; ++row)
            if (!(covered & (1u << row))) a.uncovered_rows |= 1u << row;
    } else if (!obs_only) {
        UNSUP(RS.episode_seconds || RS.episode_sums);
    }

    // reset sections
    a.reset_env = (RS.env_actions != nullptr ? 1 : 0) | (RS.episode_length != nullptr ? 2 : 0);
    if (RS.env_actions) {
        UNSUP(a.env_actions && a.env_actions != RS.env_actions);
        UNSUP(!RS.env_last_actions || (a.env_last_actions && a.env_last_actions != RS.env_last_actions));
        a.env_actions = RS.env_actions; a.env_last_actions = RS.env_last_actions;
    }
    UNSUP(RS.episode_length && RS.episode_length != T.episode_length);
    UNSUP(RS.max_episode_length && T.max_episode_length && RS.max_episode_length != T.max_episode_length);
    if (RS.max_episode_length) a.max_episode_length = RS.max_episode_length;
    a.base_max_episode_length = RS.base_max_episode_length;
    a.max_random_scaling = RS.max_episode_length ? RS.max_random_scaling : 0.0f;
    a.n_air = RS.num_contact;
    for (int m = 0; m < RS.num_contact; ++m) {
        a.air_links[m] = RS.air_links[m];
        for (int s = 0; s < 4; ++s) a.air_state[m][s] = RS.air_state[m][s];
    }
    a.reset_dofs = RS.scene_dof_pos != nullptr;
    if (RS.scene_dof_pos) {
        UNSUP(a.dof_pos && a.dof_pos != RS.scene_dof_pos);
        UNSUP(!RS.default_dof_pos || (a.default_dof_pos && a.default_dof_pos != RS.default_dof_pos));
        a.dof_pos = RS.scene_dof_pos; a.default_dof_pos = RS.default_dof_pos; a.dof_vel = RS.scene_dof_vel;
        a.dof_noise_scale = RS.dof_noise_scale;
    }
    a.scene_reset = RS.scene_pos != nullptr;
    if (RS.scene_pos) {
        const bool writes_quat = RS.spawn_mode ? RS.spawn_set_quat != 0 : RS.set_quat != 0;
        GfEntityView ev{RS.scene_pos, writes_quat ? RS.scene_quat : nullptr, RS.zero_velocity ? RS.scene_lin_vel : nullptr,
                        RS.zero_velocity ? RS.scene_ang_vel : nullptr};
        GfEntityView cur{a.pos, a.quat, a.lin_vel, a.ang_vel};
        UNSUP(!same_entity(cur, ev));
        UNSUP(writes_quat && !RS.scene_quat);
        if (RS.spawn_mode) {
            UNSUP(RS.spawn_draws);  // dense parity draws run phase by phase
            UNSUP(RS.terrain.height_field && (RS.terrain.rows < 1 || RS.terrain.cols < 1));
            UNSUP(have_terrain && memcmp(&a.terrain, &RS.terrain, sizeof(GfTerrainView)) != 0);
            a.terrain = RS.terrain;
            have_terrain = true;
            a.spawn_mode = 1; a.spawn_set_quat = RS.spawn_set_quat; a.spawn_rot_mask = RS.spawn_rot_mask;
            a.spawn_x_min = RS.spawn_x_min; a.spawn_x_span = RS.spawn_x_span; a.spawn_y_min = RS.spawn_y_min; a.spawn_y_span = RS.spawn_y_span;
            a.spawn_height_offset = RS.spawn_height_offset;
            for (int j = 0; j < 3; ++j) { a.spawn_rot_lo[j] = RS.spawn_rot_lo[j]; a.spawn_rot_hi[j] = RS.spawn_rot_hi[j]; }
        }
        UNSUP(RS.zero_velocity && (!RS.scene_lin_vel || !RS.scene_ang_vel));
        merge_entity(a, ev);
        a.set_quat = RS.set_quat; a.zero_velocity = RS.zero_velocity; a.quat_stash = RS.quat_stash;
        // the stash takes the PRE-reset quaternion out of the control wave's registers: it has to be loaded even when no term or
        // observation item of THIS launch reads it (termination done by a launch of its own, the body-frame items in an observation
        // manager that runs behind this launch, a getter the training script calls between steps) — found by the fuzz soak, seeds 123 / 140
        if (RS.quat_stash && (RS.set_quat || (RS.spawn_mode && RS.spawn_set_quat))) needs |= PN_QUAT;
        for (int j = 0; j < 3; ++j) a.reset_pos[j] = RS.reset_pos[j];
        for (int j = 0; j < 4; ++j) a.reset_quat[j] = RS.reset_quat[j];
        if (RS.zero_velocity && RS.scene_dof_vel) {
            UNSUP(a.dof_vel && a.dof_vel != RS.scene_dof_vel);
            a.dof_vel = RS.scene_dof_vel;
        }
    }

    // observations
    a.n_obs = r->num_observe;
    int omax = 0, stale_seen = 0;
    for (int m = 0; m < a.n_obs; ++m) {
        const GfObservationArgs* ob = r->observe[m];
        UNSUP(!ob || ob->num_envs != N || ob->num_items > kPostMaxItems || ob->noise_draws || !ob->obs);
        UNSUP(ob->seed != RS.seed || ob->env_offset != RS.env_offset);
        UNSUP(ob->history_ring < 0 || (int64_t)ob->history_ring > (ob->ring_slots ? (int64_t)ob->ring_slots : (int64_t)ob->history_len));
        UNSUP(ob->history_len > 1 && !ob->history_ring && !ob->prev_obs);
        UNSUP((reinterpret_cast<uintptr_t>(ob->obs) & 15u) || (ob->prev_obs && (reinterpret_cast<uintptr_t>(ob->prev_obs) & 15u)));
        GfEntityView cur{a.pos, a.quat, a.lin_vel, a.ang_vel};
        PostObs& po = a.obs[m];
        po.obs = ob->obs; po.prev = (ob->history_len > 1 && !ob->history_ring) ? ob->prev_obs : nullptr; po.stream = ob->stream;
        po.ring = ob->history_ring;
        po.ring_slots = (int32_t)ob->ring_slots;
        UNSUP(ob->ring_slots && (!ob->history_ring || (int64_t)ob->ring_slots < ob->history_len || (int64_t)ob->history_ring > (int64_t)ob->ring_slots));
        // (the frame of an in-place ring is read back by the gather that follows: cached)
        if (!po.ring && N * (int64_t)ob->obs_width * (ob->history_len > 0 ? ob->history_len : 1) * 4 >= kObsStreamBytes) a.obs_stream |= 1u << m;
        po.num_items = ob->num_items; po.width = ob->obs_width; po.history = ob->history_len;
        omax = ob->obs_width > omax ? ob->obs_width : omax;
        bool uses_entity = false;
        for (int i = 0; i < ob->num_items; ++i) {
            GfObsItem it = ob->items[i];
            switch (it.op) {
                case GF_O_COMMAND: {
                    UNSUP(it.i0 < 0 || it.i0 >= GF_MAX_COMMAND_VIEWS || !ob->command[it.i0].command || it.width != ob->command[it.i0].width);
                    const int s = pk.view_slot(ob->command[it.i0]);
                    UNSUP(s < 0);
                    UNSUP(pk.a.cmd_of_view[s] >= 0 && pk.a.cmd_of_view[s] != kViewGait && it.width > kPostMaxRanges);
                    it.i0 = s;
                } break;
                case GF_O_ANG_VEL_BODY: needs |= PN_QUAT | PN_ANG; uses_entity = true; break;
                case GF_O_LIN_VEL_BODY: needs |= PN_QUAT | PN_LIN; uses_entity = true; break;
                case GF_O_PROJ_GRAVITY: needs |= PN_QUAT; uses_entity = true; break;
                case GF_O_DOF_POS: needs |= PN_DOFPOS; UNSUP(!ob->dof_pos || (a.dof_pos && a.dof_pos != ob->dof_pos)); a.dof_pos = const_cast<float*>(ob->dof_pos); D = ob->num_dofs; break;
                case GF_O_DOF_VEL: needs |= PN_DOFVEL; UNSUP(!ob->dof_vel || (a.dof_vel && a.dof_vel != ob->dof_vel)); a.dof_vel = const_cast<float*>(ob->dof_vel); D = ob->num_dofs; break;
                case GF_O_DOF_FORCE: UNSUP(!ob->dof_force || (a.dof_force && a.dof_force != ob->dof_force)); a.dof_force = ob->dof_force; D = ob->num_dofs; break;
                case GF_O_ACTIONS: needs |= PN_TARGETS; UNSUP(!ob->targets || (a.targets && a.targets != ob->targets)); a.targets = ob->targets; D = ob->num_dofs; break;
                case GF_O_RAW_ACTIONS: needs |= PN_ACTIONS; UNSUP(!ob->env_actions || (a.env_actions && a.env_actions != ob->env_actions)); a.env_actions = const_cast<float*>(ob->env_actions); D = ob->num_dofs; break;
                case GF_O_CONTACT_FORCE_NORM: {
                    UNSUP(it.i0 < 0 || it.i0 >= GF_MAX_CONTACT_VIEWS || !ob->contact[it.i0].contacts || it.width != ob->contact[it.i0].num_links);
                    const int s = pk.contact_slot(ob->contact[it.i0]);
                    UNSUP(s < 0);
                    it.i0 = s;
                } break;
                default: return GF_E_UNSUPPORTED;
            }
            if (it.op == GF_O_DOF_POS || it.op == GF_O_DOF_VEL || it.op == GF_O_ACTIONS || it.op == GF_O_RAW_ACTIONS || it.op == GF_O_DOF_FORCE)
                UNSUP(it.width != ob->num_dofs);
            po.items[i] = it;
        }
        if (uses_entity) {
            UNSUP(!same_entity(cur, ob->entity));
            merge_entity(a, ob->entity);
            // stale quaternion source must be this step's reset (or absent when the reset does not touch quat)
            if (obs_only) {
                // the reset ran (or, in a step without a done env, did not run) as a launch of its own: the manager's descriptor says
                // whether this tick has a stash to read, and every manager of the launch must say the same
                UNSUP(ob->stale_quat && (ob->stale_quat != RS.quat_stash || ob->stale_mask != T.terminated || ob->stale_mask2 != T.truncated));
                stale_seen |= ob->stale_quat ? 1 : 2;
            } else if (a.scene_reset && (a.spawn_mode ? a.spawn_set_quat : a.set_quat)) {
                UNSUP(ob->stale_quat != a.quat_stash || ob->stale_mask != T.terminated || ob->stale_mask2 != T.truncated);
            } else {
                UNSUP(ob->stale_quat != nullptr);
            }
        }
    }
    if (obs_only) {
        UNSUP(stale_seen == 3);
        a.quat_stash = (stale_seen & 1) ? RS.quat_stash : nullptr;
    }
    UNSUP(omax >= GF_MAX_OBS_WIDTH);

    // rollout-storage rows (§8f-5): second stores of what the launch holds anyway
    if (const GfRolloutArgs* ro = r->rollout) {
        UNSUP(ro->num_envs != N);
        UNSUP((ro->done_out && (ro->terminated != T.terminated || ro->truncated != T.truncated)) || (ro->reward_out && (!RW || ro->reward != RW->reward)));
        a.roll_reward = ro->reward_out; a.roll_done = ro->done_out;
        a.roll_obs = nullptr; a.roll_obs_index = -1;
        if (ro->obs_out) {
            for (int m = 0; m < a.n_obs; ++m)
                if (a.obs[m].obs == ro->obs && a.obs[m].width * a.obs[m].history == ro->obs_width) a.roll_obs_index = m;
            UNSUP(a.roll_obs_index < 0 || (reinterpret_cast<uintptr_t>(ro->obs_out) & 15u));
            UNSUP(a.obs[a.roll_obs_index].ring != 0);   // an in-place ring is not a newest-first row: nothing to copy from
            a.roll_obs = ro->obs_out;
        }
    }

    // everything the kernel dereferences must exist, be float4-aligned and agree on D
    a.num_dofs = D > 0 ? D : 4;   // (no phase of the launch reads a DOF row — possible in front of a reset that user code runs: one unused chunk)
    a.needs = needs;
    UNSUP((needs & PN_QUAT) && !a.quat);
    UNSUP((needs & PN_POS) && !a.pos);
    UNSUP((needs & PN_LIN) && !a.lin_vel);
    UNSUP((needs & PN_ANG) && !a.ang_vel);
    UNSUP((needs & PN_EPLEN) && !a.episode_length);
    // DOF rows are ceil(D / 4) float4 chunks (a last chunk of fewer than four floats is handled element by element, gf_post_args.h):
    // 12 and 28 DOF have static programs, every count up to 32 an interpreter variant
    const bool dofs_ok = D >= 1 && D <= 32;
    UNSUP((needs & (PN_DOFPOS | PN_DOFVEL | PN_TARGETS | PN_ACTIONS | PN_LAST)) && !dofs_ok);
    UNSUP((a.reset_dofs || (a.reset_env & 1)) && !dofs_ok);
    UNSUP((needs & PN_DOFPOS) && !a.dof_pos);
    UNSUP((needs & PN_DOFVEL) && !a.dof_vel);
    UNSUP((needs & PN_TARGETS) && !a.targets);
    UNSUP((needs & PN_ACTIONS) && !a.env_actions);
    UNSUP((needs & PN_LAST) && !a.env_last_actions);
    UNSUP((needs & PN_DOFDEV) && !a.default_dof_pos);
    const void* al[] = {a.quat, a.dof_pos, a.dof_vel, a.targets, a.env_actions, a.env_last_actions, a.default_dof_pos, a.quat_stash, a.dof_force};
    for (const void* p : al) UNSUP(reinterpret_cast<uintptr_t>(p) & 15u);
    UNSUP((int64_t)N * (D > 4 ? D : 4) * 4 >= (int64_t)1 << 32);
    return GF_OK;
}


// ---- the scene's ContactManagers in front of the other phases, in the same launch (GfPostArgs.cfold) ------------------------------
int validate_contact(const GfContactArgs* a);                                   // gf_contact.hip
bool contact_compatible(const GfContactArgs* x, const GfContactArgs* y);
ContactMgrL contact_mgr_image(const GfContactArgs* a);

// GF_OK: pk.a.cfold describes the managers and the launch runs their step first; GF_E_UNSUPPORTED: the caller launches the contact
// kernel itself (more than 32 tracked links / 16 with-filter links / 255 scene links, slot rows that do not fit the tile's LDS,
// a statistics block other than the step's, an observation-only launch, GF_OPT_FOLD_CONTACT = 0).
static int fold_contacts(Packer& pk, const GfContactArgs* const* mgrs, int num) {
    GfPostArgs& a = pk.a;
    UNSUP(!g_options[GF_OPT_FOLD_CONTACT]);
    UNSUP(num < 1 || num > kFoldMaxMgr || a.obs_only);
    PostContact& f = a.cfold;
    int total = 0;
    for (int m = 0; m < num; ++m) {
        const GfContactArgs* c = mgrs[m];
        const int rc = validate_contact(c);
        if (rc) return rc;
        UNSUP(m > 0 && !contact_compatible(mgrs[0], c));
        UNSUP(c->num_envs != a.num_envs || c->num_contacts < 1 || c->num_scene_links > 255);
        UNSUP(total + c->num_targets > kFoldMaxTargets || c->num_with > kFoldMaxWith);
        UNSUP(c->stats && c->stats != a.stats);
        const ContactMgrL l = contact_mgr_image(c);
        PostContactMgr& o = f.m[m];
        o.contacts = l.contacts; o.contact_positions = l.contact_positions; o.position_counts = l.position_counts;
        o.link_vel_out = l.link_vel_out; o.link_pos_out = l.link_pos_out;
        o.last_air_time = l.last_air_time; o.current_air_time = l.current_air_time;
        o.last_contact_time = l.last_contact_time; o.current_contact_time = l.current_contact_time;
        o.air_time_threshold = l.air_time_threshold;
        o.num_targets = (uint8_t)l.num_targets; o.num_with = (uint8_t)l.num_with;
        o.has_with_filter = l.has_with_filter ? 1 : 0; o.track_air_time = l.track_air_time ? 1 : 0;
        for (int w = 0; w < c->num_with; ++w) {
            UNSUP(c->with_link_ids[w] < 0 || c->with_link_ids[w] > 254);
            o.with_ids[w] = (uint8_t)c->with_link_ids[w];
        }
        for (int t = 0; t < c->num_targets; ++t) {
            UNSUP(c->target_link_ids[t] < 0 || c->target_link_ids[t] > 254);
            f.target_ids[total] = (uint8_t)c->target_link_ids[t];
            f.mgr_of[total] = (uint8_t)m;
            f.local_of[total] = (uint8_t)t;
            ++total;
        }
    }
    const GfContactArgs* c0 = mgrs[0];
    UNSUP(fold_lds_bytes(c0->num_contacts) + sizeof(GfPostArgs) > 60 * 1024);
    // Measured on one box with the fold as shipped and switched off (tools/scaling_table.sh, profiles/r04_t_scaling.jsonl; us per step):
    //   one pass of the tile's 256 lanes (up to 4 tracked links: humanoid 3, contacts 4)  8 192 … 1 024 envs: 24.7 / 23.1 / 22.8 / 22.6 vs 26.6 / 26.6 / 25.3 / 25.0
    //   three passes (rough terrain, 9 links)   16 384 / 8 192 / 4 096 / 2 048 envs: 32.0 / 27.4 / 25.1 / 25.1 vs 31.6 / 25.5 / 25.8 / 25.2
    //   four passes (gait task, 13 links)       65 536 / 32 768 / 16 384 / 8 192 envs: 118.2 / 73.4 / 51.0 / 39.9 vs 125.5 / 77.2 / 50.3 / 39.3
    // A tile that needs several passes pays them one after the other on ONE CU, where a launch of its own spreads the same pairs over
    // four times as many small workgroups: below these sizes (128-256 tiles on 256 CUs) that costs more than the launch it saves.
    // GF_OPT_FOLD_CONTACT = 2 folds regardless.
    const int passes = (total * kEnvBlock + kWsBlock - 1) / kWsBlock;
    const int min_envs = passes >= 4 ? 32768 : (passes >= 2 ? 16384 : 0);
    UNSUP(g_options[GF_OPT_FOLD_CONTACT] != 2 && a.num_envs < min_envs);
    f.force = c0->force; f.position = c0->position; f.links_quat = c0->links_quat; f.links_vel = c0->links_vel; f.links_pos = c0->links_pos;
    f.link_a = c0->link_a; f.link_b = c0->link_b;
    f.num_contacts = c0->num_contacts; f.num_scene_links = c0->num_scene_links; f.num_mgr = num; f.total_targets = total;
    f.dt = c0->dt;
    return GF_OK;
}

}  // namespace gf

extern "C" __attribute__((visibility("default"))) int gf_post_physics_check(const GfPostRefs* r) {
    gf::Packer pk;
    return gf::pack(r, pk);
}

static_assert(gf::PN_POS == GF_POST_NEEDS_POS && gf::PN_QUAT == GF_POST_NEEDS_QUAT && gf::PN_LIN == GF_POST_NEEDS_LIN && gf::PN_ANG == GF_POST_NEEDS_ANG &&
              gf::PN_DOFPOS == GF_POST_NEEDS_DOFPOS && gf::PN_DOFVEL == GF_POST_NEEDS_DOFVEL && gf::PN_TARGETS == GF_POST_NEEDS_TARGETS &&
              gf::PN_ACTIONS == GF_POST_NEEDS_ACTIONS && gf::PN_LAST == GF_POST_NEEDS_LAST && gf::PN_EPLEN == GF_POST_NEEDS_EPLEN &&
              gf::PN_MAXLEN == GF_POST_NEEDS_MAXLEN && gf::PN_DOFDEV == GF_POST_NEEDS_DOFDEV && gf::PN_ACTRATE == GF_POST_NEEDS_ACTRATE &&
              gf::PN_DOFFORCE == GF_POST_NEEDS_DOFFORCE, "gf_step.h names the kernel's bits");
extern "C" __attribute__((visibility("default"))) int gf_post_physics_needs(const GfPostRefs* r, uint32_t* needs_out) {
    if (!needs_out) return GF_E_NULL;
    gf::Packer pk;
    const int rc = gf::pack(r, pk);
    if (rc) return rc;
    *needs_out = pk.a.needs;
    return GF_OK;
}

// ------------------------------------------------------------------------------------------------------------
// The program table: everything the host knows about a program of the fused launch is one PostProgram record.
// ------------------------------------------------------------------------------------------------------------
namespace gf {

struct PostProgram {
    int id;                                  // 0: table interpreter, 1…: built-in, kDynBase…: compiled at run time
    const char* name;
    int (*matches)(const GfPostArgs*);       // built-in / run-time programs; an interpreter row is picked by DOF count (interp_program)
    const void* kernel;                      // post_ws_kernel<P>
    size_t (*lds_bytes)(int omax, int n_gait);   // everything the program itself needs, the interpreter's descriptor copy included
    bool keeps_args_in_lds;                  // interpreter: a folded contact phase stages its slots behind the descriptor copy
    bool folds;                              // ws_prog_folds<P>(): the kernel carries the contact phase
    const void* tick_kernel;                 // post_ws_kernel_tick<P>; nullptr: the program has no tick variant
    size_t (*tick_lds_bytes)(int omax, int n_gait);
};

template <class P>
static size_t program_lds_bytes(int omax, int n_gait) {
    return (P::kStatic ? 0 : sizeof(GfPostArgs)) + lds_ws_floats<P>(omax, n_gait) * sizeof(float);
}
// kWithTick instantiates post_ws_kernel_tick<P> (a kernel of its own, as large as post_ws_kernel<P>): named per program, on purpose.
// The tick prologue covers static programs 1 and 2 and the 12- / 28-DOF table interpreter; the other built-in programs (contact
// phases, per-link rows: scenes the tick variant does not cover) and every program compiled at run time keep their own launch.
template <class P, bool kWithTick = false>
static PostProgram make_program(int id) {
    PostProgram p{};
    p.id = id;
    if constexpr (P::kStatic) {
        p.name = P::name;
        p.matches = [](const GfPostArgs* a) -> int { return program_matches<P>(*a); };
    } else {
        p.name = "interpreter";
    }
    p.kernel = reinterpret_cast<const void*>(&post_ws_kernel<P>);
    p.lds_bytes = program_lds_bytes<P>;
    p.keeps_args_in_lds = !P::kStatic;
    p.folds = ws_prog_folds<P>();
    if constexpr (kWithTick) {
        p.tick_kernel = reinterpret_cast<const void*>(&post_ws_kernel_tick<P>);
        p.tick_lds_bytes = program_lds_bytes<WithTick<P>>;
    }
    return p;
}

// Built-in programs in registration order: the first that matches runs.  tools/register_program.py --write appends to this list.
static const PostProgram kBuiltin[] = {
    make_program<ProgGo2CommandDirection, true>(1),
    make_program<ProgGo2Simple, true>(2),
    make_program<ProgGo2Contacts>(3),
    make_program<ProgGo2RoughTerrain>(4),
    make_program<ProgBerkeleyHumanoid>(5),
    make_program<ProgGo2GaitTrainer>(6),
    make_program<ProgHumanoid28Stress>(7),
    make_program<ProgGo2GaitTrainerFront>(8),
    make_program<ProgGo2GaitTrainerObs>(9),
};

// The table interpreter, one kernel per (float4 chunks of a DOF row, short last chunk): row [chunks - 1][tail].  Chunks 1 … 8 are the
// DOF counts 1 … 32 that pack() admits for a step that reads a DOF row; chunk 3 serves 9 … 11 (tail) and 12.
static const PostProgram kInterp[8][2] = {
    {make_program<Interp<1, false>>(0), make_program<Interp<1, true>>(0)},
    {make_program<Interp<2, false>>(0), make_program<Interp<2, true>>(0)},
    {make_program<Interp<3, false>, true>(0), make_program<Interp<3, true>>(0)},
    {make_program<Interp<4, false>>(0), make_program<Interp<4, true>>(0)},
    {make_program<Interp<5, false>>(0), make_program<Interp<5, true>>(0)},
    {make_program<Interp<6, false>>(0), make_program<Interp<6, true>>(0)},
    {make_program<Interp<7, false>, true>(0), make_program<Interp<7, true>>(0)},
    {make_program<Interp<8, false>>(0), make_program<Interp<8, true>>(0)},
};
static const PostProgram& interp_program(int num_dofs) {
    // pack() turns "no phase reads a DOF row" into 4; a count above 32 gets past it only in such a step and runs the 12-DOF row
    if (num_dofs < 1 || num_dofs > 32) num_dofs = 12;
    return kInterp[(num_dofs + 3) / 4 - 1][num_dofs % 4 != 0];
}

// ---- programs compiled at run time (include/gf_step.h: gf_post_program_register) ---------------------------------------------
// A plugin is a small shared object built from csrc/gf_post_ws.h + ONE generated program struct (genesis_forge_amd/_programs.py):
// it carries post_ws_kernel<P> in its own code object and exports the matcher, the kernel's host handle and its LDS size.  The
// library only keeps their records; ids start at kDynBase.  Registration is rare and append-only (fixed-size table, the count is
// published last), selection walks it on every launch of a config no built-in program matches.
constexpr int kDynBase = 100, kDynMax = 256;   // (programs registered per process)
static PostProgram g_dyn[kDynMax];
static char g_dyn_name[kDynMax][64];
static std::atomic<int> g_dyn_count{0};
static std::mutex g_dyn_mutex;

constexpr size_t kPostLaunchLdsMax = 160 * 1024;   // hipDeviceProp_t::sharedMemPerBlock of an MI355X: what a plain launch takes
static int post_omax(const GfPostArgs& a) {         // the widest single frame of the launch's observation managers
    int omax = 0;
    for (int m = 0; m < a.n_obs; ++m) omax = a.obs[m].width > omax ? a.obs[m].width : omax;
    return omax;
}

static const PostProgram& select_program(const GfPostArgs& a) {
    if (g_options[GF_OPT_POST_VARIANT] >= 2) {
        for (const PostProgram& p : kBuiltin)
            if (p.matches(&a)) return p;
        // A program compiled at run time parks one LDS row per link of every contact-force-norm item on top of the tile (two managers of
        // 255 norm columns: 510 rows, 128 KiB): one that would ask for more than a workgroup has is passed over, and the interpreter —
        // whose request is bounded for every descriptor pack() admits (post_lds_bytes) — runs the step.  The built-in programs' matchers
        // pin their widths.
        const int n = g_dyn_count.load();
        for (int i = 0; i < n; ++i)
            if (g_dyn[i].matches(&a) && g_dyn[i].lds_bytes(post_omax(a), a.n_gait) <= kPostLaunchLdsMax) return g_dyn[i];
    }
    return interp_program(a.num_dofs);
}

// the action and scene ops of a step that run as the launch's tick prologue (post_ws_kernel_tick)
struct TickLaunch {
    const GfActionArgs* act;
    const GfSynthSceneArgs* scene;
    int upkeep;
};
// The dynamic LDS of one launch of program `p` on the packed descriptor `a`.  post_launch() hands it to the launch as it is — no
// attribute is set on the kernel: gfx950 takes up to kPostLaunchLdsMax per workgroup from a plain launch (measured,
// profiles/post_capacity.md).  The largest request a descriptor pack() admits is the 32-DOF interpreter at a 255-wide frame with a
// gait manager: sizeof(GfPostArgs) + (37 + 16 + 32 + 256) rows of 64 floats, about 89 KiB; the static_assert below holds the bound
// for every interpreter row, tick variants included (tests/test_post_capacity.py asserts the same through gf_post_interp_lds_bytes).
static size_t post_lds_bytes(const GfPostArgs& a, const PostProgram& p, bool tick) {
    const int omax = post_omax(a);
    // a folded contact phase stages the tile's slot ids in the LDS the later phases use (behind the interpreter's descriptor copy)
    const size_t fold_lds = a.cfold.num_mgr > 0 ? fold_lds_bytes(a.cfold.num_contacts) + (p.keeps_args_in_lds ? sizeof(GfPostArgs) : 0) : 0;
    const size_t own_lds = (tick && p.tick_lds_bytes ? p.tick_lds_bytes : p.lds_bytes)(omax, a.n_gait);
    return own_lds > fold_lds ? own_lds : fold_lds;
}
static_assert(sizeof(GfPostArgs) + (size_t)(x_fields(1) + kPostMaxReward + kPostAuxRows + GF_MAX_OBS_WIDTH) * kEnvBlock * sizeof(float) <= kPostLaunchLdsMax &&
              sizeof(GfPostArgs) + (size_t)(x_fields(1) + kPostMaxReward) * kEnvBlock * sizeof(float) + (size_t)ws_hand_floats<Interp<8, false>>() * sizeof(float) <= kPostLaunchLdsMax,
              "the widest frame pack() admits (GF_MAX_OBS_WIDTH - 1 columns + the tile's pad column) at 32 DOF fits a workgroup's LDS");

// launches the post-physics kernel of program `p`; with `tick`, its tick variant (p.tick_kernel, the caller has looked)
static int post_launch(const GfPostArgs& packed, hipStream_t s, const PostProgram& p, const TickLaunch* tick = nullptr) {
#ifdef GF_STAMPS
    GfPostArgs stamped = packed;
    stamped.stamps = gf_debug_stamps;
    const uint32_t stamp_tiles = (uint32_t)env_grid(packed.num_envs);
    stamped.stamp_stride = stamp_tiles / kStampSlots > 0 ? stamp_tiles / kStampSlots : 1u;
    const char* const rs = getenv("GF_ROLE_SHIFT");   // (read per launch)
    stamped.role_shift = rs && *rs >= '0' && *rs <= '9' && atoi(rs) <= 15 ? atoi(rs) : -1;
    const GfPostArgs& a = stamped;
#else
    const GfPostArgs& a = packed;
#endif
    const size_t lds = post_lds_bytes(a, p, tick != nullptr);
    const dim3 grid(env_grid(a.num_envs) + (unsigned)(tick ? tick->upkeep : 0)), block(kWsBlock);
    const void* const kernel = tick ? p.tick_kernel : p.kernel;
    void* kargs[4] = {const_cast<GfPostArgs*>(&a), nullptr, nullptr, nullptr};   // (post_ws_kernel reads the first only)
    if (tick) {
        kargs[1] = const_cast<GfActionArgs*>(tick->act);
        kargs[2] = const_cast<GfSynthSceneArgs*>(tick->scene);
        kargs[3] = const_cast<int*>(&tick->upkeep);
    }
    PhaseScope scope(GF_PHASE_POST, s);   // (never active with a tick: step_fold_try leaves a profiled phase its own launch)
    if (scope.active()) {
        scope.use_dispatch_events();
        (void)hipExtLaunchKernel(kernel, grid, block, kargs, lds, s, scope.start(), scope.stop(), 0);
    } else {
        sink_launch(kernel, grid, block, lds, s, kargs);
    }
    return launch_status();
}

int action_scene_check(const GfActionArgs* act, const GfSynthSceneArgs* a, int* rc, ActionScenePlan* plan);   // gf_scene.hip
int action_scene_launch(const GfActionArgs* act, const GfSynthSceneArgs* a, const ActionScenePlan& p, hipStream_t s);

int post_step(const GfPostRefs* r, const GfContactArgs* const* mgrs, int num_mgr, hipStream_t s) {
    Packer pk;
    int rc = pack(r, pk);
    if (rc) return rc;
    const PostProgram& p = select_program(pk.a);
    if (num_mgr > 0) {
        UNSUP(!p.folds);   // the kernel this descriptor selects does not carry the contact phase
        rc = fold_contacts(pk, mgrs, num_mgr);
        if (rc) return rc;
    }
    return post_launch(pk.a, s, p);
}

// gf_run_ops, the ops of a recorded step on the stand-in scene in a row — action, scene, post-physics: ONE launch, the post-physics kernel
// with the tile's tick as its prologue.  Returns the number of ops that are done:
//   0: nothing enqueued or reported — the caller goes on as if this peephole did not exist (an op is invalid, the pair does not fold, a
//      switch is off: the action / scene pair and the post-physics op run, fold and fail as they always did);
//   2: the pair is done in its own launch, as action_scene_try does it (*rc its status); the post-physics op is the caller's — a scene
//      with per-link rows or contact slots, or a post-physics op that does not pack (it then fails, or runs unfused, with its own index);
//   3: all three are done (*rc the status of the last launch): in one launch, or — the packed step is out of the fold's scope, the
//      selected program has no tick variant — in the two launches of the unfolded step, without validating and packing twice.
// What is on the stream after an error and the index it is reported with are the same in every case.
// GF_FOLD_STEP=0 switches the peephole off (A/B runs, tests/test_step_fold.py); read per call.
static std::atomic<long> g_step_folds{0};
int step_fold_try(const GfActionArgs* act, const GfSynthSceneArgs* sc, const GfPostRefs* refs, hipStream_t s, int* rc) {
    const char* sw = getenv("GF_FOLD_STEP");
    if (sw && strcmp(sw, "0") == 0) return 0;
    if (g_prof.phase == GF_PHASE_POST) return 0;   // a profiled phase keeps its own launch (… ACTION, SCENE: action_scene_check)
    ActionScenePlan plan;
    int vrc = GF_OK;
    if (action_scene_check(act, sc, &vrc, &plan) != 3) return 0;
    Packer pk;
    if (plan.links || plan.contacts || pack(refs, pk) != GF_OK) {
        *rc = action_scene_launch(act, sc, plan, s);
        return 2;
    }
    const GfPostArgs& a = pk.a;
    // what the post-physics phase reads of the arrays the tick writes, it reads of ITS tile: the same arrays, row for row
    auto same = [](const void* p, const void* q) { return !p || p == q; };
    const bool in_scope = a.num_envs == sc->num_envs && a.num_dofs == sc->num_dofs &&
                          // block 0 of a launch that reads the gait manager's per-block bytes is its tile 0 (gf_terms.h), and a launch with
                          // a gait manager writes one byte per block: not with upkeep workgroups in front
                          a.n_gait == 0 && !a.gait_wave_flags &&
                          same(a.pos, sc->pos) && same(a.quat, sc->quat) && same(a.lin_vel, sc->lin_vel) && same(a.ang_vel, sc->ang_vel) &&
                          same(a.dof_pos, sc->dof_pos) && same(a.dof_vel, sc->dof_vel) && same(a.targets, sc->targets) &&
                          same(a.env_actions, act->env_actions) && same(a.env_last_actions, act->env_last_actions) &&
                          same(a.episode_length, act->episode_length);
    const PostProgram& p = select_program(a);
    if (in_scope && p.tick_kernel) {
        const TickLaunch tick{act, sc, plan.upkeep};
        *rc = post_launch(a, s, p, &tick);
        g_step_folds.fetch_add(1, std::memory_order_relaxed);
        return 3;
    }
    if ((*rc = action_scene_launch(act, sc, plan, s)) != GF_OK) return 2;
    *rc = post_launch(a, s, p);
    return 3;
}

}  // namespace gf

extern "C" __attribute__((visibility("default"))) int gf_post_program_register(const char* path, int* id_out) {
    using namespace gf;
    if (!path) return GF_E_NULL;
    void* dl = dlopen(path, RTLD_NOW | RTLD_LOCAL);
    if (!dl) return GF_E_UNSUPPORTED;
    auto abi = (int (*)(void))dlsym(dl, "gfp_abi_version");
    auto asz = (int (*)(void))dlsym(dl, "gfp_args_size");
    auto nm = (const char* (*)(void))dlsym(dl, "gfp_name");
    auto mt = (int (*)(const GfPostArgs*))dlsym(dl, "gfp_matches");
    auto kn = (const void* (*)(void))dlsym(dl, "gfp_kernel");
    auto ld = (size_t (*)(int, int))dlsym(dl, "gfp_lds_bytes");
    // the packed descriptor is the interface between library and plugin: both must come from the same headers
    if (!abi || !asz || !nm || !mt || !kn || !ld || abi() != GF_ABI_VERSION || asz() != (int)sizeof(GfPostArgs)) {
        dlclose(dl);
        return GF_E_UNSUPPORTED;
    }
    std::lock_guard<std::mutex> lock(g_dyn_mutex);
    const int n = g_dyn_count.load();
    for (int i = 0; i < n; ++i)
        if (!strncmp(g_dyn_name[i], nm(), sizeof(g_dyn_name[i]) - 1)) {   // already there (same signature hash in the name)
            dlclose(dl);
            if (id_out) *id_out = kDynBase + i;
            return GF_OK;
        }
    if (n >= kDynMax) { dlclose(dl); return GF_E_RANGE; }
    snprintf(g_dyn_name[n], sizeof(g_dyn_name[n]), "%s", nm());
    auto fo = (int (*)(void))dlsym(dl, "gfp_folds");   // the plugin's kernel carries the contact phase (ws_prog_folds<P>)
    g_dyn[n] = PostProgram{kDynBase + n, g_dyn_name[n], mt, kn(), ld, false, fo && fo() != 0, nullptr, nullptr};   // (the plugin stays loaded)
    g_dyn_count.store(n + 1);
    if (id_out) *id_out = kDynBase + n;
    return GF_OK;
}

extern "C" __attribute__((visibility("default"))) int gf_post_program_count(void) { return gf::g_dyn_count.load(); }

extern "C" __attribute__((visibility("default"))) int gf_post_physics_describe(const GfPostRefs* r, char* buf, int cap) {
    gf::Packer pk;
    const int rc = gf::pack(r, pk);
    if (rc) return rc;
    if (!buf || cap <= 0) return GF_E_NULL;
    const gf::PostProgram& p = gf::select_program(pk.a);
    int n = snprintf(buf, (size_t)cap, "program %d (%s): ", p.id, p.name);
    if (n < cap) gf::describe_program(pk.a, buf + n, cap - n);
    return GF_OK;
}

// Host-only, like gf_post_physics_check: the dynamic LDS post_launch() would ask for on these descriptors (the program selected under
// the current GF_OPT_POST_VARIANT; `tick`: its tick variant where it has one), without a folded contact phase.
extern "C" __attribute__((visibility("default"))) int gf_post_physics_lds_bytes(const GfPostRefs* r, int tick, long* bytes_out) {
    if (!bytes_out) return GF_E_NULL;
    gf::Packer pk;
    const int rc = gf::pack(r, pk);
    if (rc) return rc;
    *bytes_out = (long)gf::post_lds_bytes(pk.a, gf::select_program(pk.a), tick != 0);
    return GF_OK;
}

// … and of the table interpreter's row for `num_dofs` at a single-frame width `omax` (the capacity bound: no descriptor needed)
extern "C" __attribute__((visibility("default"))) long gf_post_interp_lds_bytes(int num_dofs, int omax, int n_gait, int tick) {
    const gf::PostProgram& p = gf::interp_program(num_dofs);
    return (long)(tick && p.tick_lds_bytes ? p.tick_lds_bytes : p.lds_bytes)(omax, n_gait);
}

// steps gf_run_ops ran as one launch since the library was loaded (tests: the fold took place)
extern "C" __attribute__((visibility("default"))) long gf_step_fold_count(void) { return gf::g_step_folds.load(std::memory_order_relaxed); }

extern "C" __attribute__((visibility("default"))) int gf_post_physics_step(const GfPostRefs* r, void* stream) {
    return gf::post_step(r, nullptr, 0, (hipStream_t)stream);
}

extern "C" __attribute__((visibility("default"))) int gf_post_physics_step_contacts(const GfPostRefs* r, const GfContactArgs* const* contacts, int num_contacts,
                                                                                   void* stream) {
    if (num_contacts < 0 || (num_contacts > 0 && !contacts)) return GF_E_NULL;
    return gf::post_step(r, contacts, num_contacts, (hipStream_t)stream);
}
