// c3d_step_kinds.h — what the `kind` of a step (DevStep::kind, Step64::kind) and of a stage (c3d_stage::kind) is: the names of the nine
// values and the facts about a kind that kernels and host ask for, each said once.  Included by c3d_internal.h, so every host and
// device unit sees it.  The numbers are ABI (include/c3d.h documents them; DevStep and Step64 carry them as plain ints into the kernels,
// and build_program run-length codes the structs with memcmp): a new kind gets a new number, a name here and its line in every predicate
// it belongs to.
#pragma once

namespace c3d {

enum StepKind : int {
    kMdCouple = 0,         // MD step, temperature coupling
    kMdRescale = 1,        // MD step, velocity rescale
    kFire = 2,             // FIRE step
    kFireFirst = 3,        // first FIRE step of a stage: fresh state, no incoming velocity
    kMdBegin = 4,          // MD begin: takes the Maxwell velocities, no force, no move
    kTwoPoint = 5,         // two-point step-size (Barzilai-Borwein) minimiser step
    kTwoPointFirst = 6,    // its first step of a stage
    kLbfgs = 8,            // L-BFGS step (k_lbfgs_eval + k_lbfgs_move only: never k_step / k_cluster)
    kLbfgsFirst = 9,       // its first step of a stage
};
static_assert(kMdCouple == 0, "c3d.h documents the numbers");
static_assert(kMdRescale == 1, "c3d.h documents the numbers");
static_assert(kFire == 2, "c3d.h documents the numbers");
static_assert(kFireFirst == 3, "c3d.h documents the numbers");
static_assert(kMdBegin == 4, "c3d.h documents the numbers");
static_assert(kTwoPoint == 5, "c3d.h documents the numbers");
static_assert(kTwoPointFirst == 6, "c3d.h documents the numbers");
static_assert(kLbfgs == 8, "c3d.h documents the numbers");
static_assert(kLbfgsFirst == 9, "c3d.h documents the numbers");

// The facts.  A kernel whose machine code a call would change keeps the fact written out at that site, with the names (the fp32 step
// controller and row update, k_step's body, k_update_sym, k_cluster: profiles/r33_step_kinds.md lists the sites); such a site changes
// with the fact it spells.
#define C3D_KIND_FACT __host__ __device__ constexpr bool
// the four families
C3D_KIND_FACT kind_is_md(int kind) { return kind == kMdCouple || kind == kMdRescale || kind == kMdBegin; }
C3D_KIND_FACT kind_is_fire(int kind) { return kind == kFire || kind == kFireFirst; }
C3D_KIND_FACT kind_is_two_point(int kind) { return kind == kTwoPoint || kind == kTwoPointFirst; }
C3D_KIND_FACT kind_is_lbfgs(int kind) { return kind == kLbfgs || kind == kLbfgsFirst; }
// the first step of a minimiser's run in a stage
C3D_KIND_FACT kind_is_first(int kind) { return kind == kFireFirst || kind == kTwoPointFirst || kind == kLbfgsFirst; }
// the step's controller is formed from the previous step's replica sums (the other kinds read none)
C3D_KIND_FACT kind_reads_sums(int kind) { return kind == kMdCouple || kind == kMdRescale || kind == kFire || kind == kTwoPoint; }
// the step goes on from the controller state the previous step stored (a first step starts from the FIRE values)
C3D_KIND_FACT kind_continues_state(int kind) { return kind == kFire || kind == kTwoPoint; }
// the step stores its controller state for the next one
C3D_KIND_FACT kind_stores_state(int kind) { return kind == kFire || kind == kFireFirst || kind == kTwoPoint || kind == kTwoPointFirst; }
// the step has no incoming velocity: the slot is not read
C3D_KIND_FACT kind_has_no_velocity(int kind) { return kind == kFireFirst || kind == kTwoPointFirst; }
#undef C3D_KIND_FACT

// host side, the public stage kinds (c3d_stage::kind): a minimiser stage — its steps are FIRE, two-point or L-BFGS steps and the exit
// test applies to it — against an MD stage
constexpr bool stage_is_minimiser(int stage_kind) { return stage_kind == kFire || stage_kind == kTwoPoint || stage_kind == kLbfgs; }

}  // namespace c3d
