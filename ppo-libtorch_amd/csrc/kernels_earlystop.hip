// Early stop at a target KL, decided on the device (ppo_target_kl_set; the reference's loop is CleanRL's minus `if approx_kl > target_kl: break`,
// PPO_Discrete.cpp:567-644).  Two one-workgroup kernels, launched by ppo_update only while a target is set:
//   kl_gate_kernel      behind the optimizer launch of the last minibatch of epoch e: reads that step's approx_kl (:352) out of its StepStats and, when it
//                       exceeds the target, raises PPO_ERRFLAG_KL_STOP in the context's error word -- the optimizer kernels do not apply a step behind it
//                       (PPO_ERRFLAG_SKIP_STEP) -- and saves what the unapplied steps overwrite: the statistics of the last applied step and the clipfrac sums.
//   kl_gate_end_kernel  at the end of the update: restores the saved statistics into the slot the host reads, clears the bit, and completes the outcome
//                       (the head of EarlyStopDev) that ppo_update copies into a pinned block behind it, for ppo_early_stop_read and for the next
//                       update's AdamW step count.
// One workgroup of one thread each (a few dozen bytes of work); the launches exist for their place in the stream.
#include "ppo_internal.hpp"

__global__ __launch_bounds__(1) void kl_gate_kernel(const StepStats* __restrict__ step_stat, double target, int epoch, double* clipfrac_accum,
                                                    int32_t* error_flag, EarlyStopDev* es) {
    if (epoch == 0) { es->stopped = 0; es->epochs_run = 0; es->kl_at_stop = 0.0; }   // the update's first gate opens its record
    else if (es->stopped) return;                                                      // epochs behind the stop were not applied: nothing to judge
    const double kl = step_stat->approx_kl;
    if (kl > target) {   // NaN compares false, as `approx_kl > target_kl` does
        es->stopped = 1;
        es->epochs_run = epoch + 1;
        es->kl_at_stop = kl;
        es->saved = *step_stat;
        es->cf[0] = clipfrac_accum[0]; es->cf[1] = clipfrac_accum[1];
        atomicOr(error_flag, PPO_ERRFLAG_KL_STOP);
    }
}

__global__ __launch_bounds__(1) void kl_gate_end_kernel(StepStats* __restrict__ last_stat, double* clipfrac_accum, int32_t* error_flag, EarlyStopDev* es,
                                                        int epochs, int n_mb, long long applied_before) {
    if (es->stopped) {
        *last_stat = es->saved;
        clipfrac_accum[0] = es->cf[0]; clipfrac_accum[1] = es->cf[1];
        atomicAnd(error_flag, ~PPO_ERRFLAG_KL_STOP);   // other kernels OR error bits into this word
    } else {
        es->epochs_run = epochs;
    }
    es->applied_total = applied_before + (long long)es->epochs_run * n_mb;   // the host knows the steps applied before this update, the device this update's
}

hipError_t launch_kl_gate(const StepStats* step_stat, double target, int epoch, double* clipfrac_accum, int32_t* error_flag, EarlyStopDev* es, hipStream_t s) {
    if (!step_stat || !clipfrac_accum || !error_flag || !es) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kl_gate_kernel, dim3(1), dim3(1), 0, s, step_stat, target, epoch, clipfrac_accum, error_flag, es);
    return hipGetLastError();
}

hipError_t launch_kl_gate_end(StepStats* last_stat, double* clipfrac_accum, int32_t* error_flag, EarlyStopDev* es, int epochs, int n_mb, int64_t applied_before,
                              hipStream_t s) {
    if (!last_stat || !clipfrac_accum || !error_flag || !es) return hipErrorInvalidValue;
    hipLaunchKernelGGL(kl_gate_end_kernel, dim3(1), dim3(1), 0, s, last_stat, clipfrac_accum, error_flag, es, epochs, n_mb, (long long)applied_before);
    return hipGetLastError();
}
