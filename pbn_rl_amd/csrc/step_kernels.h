// step_kernels.h -- the device side of libpbn_env.so: the step / rollout / reset / histogram
// kernels and their helpers (library-internal).  Included by pbn_env.hip (host side, the
// one-update instances) and pbn_settle.hip (the settle-law instances), so the two halves of
// the template instances compile in parallel.
// The per-env half of the transition law (ext64 and the bounded draws, the perturbation mask, the
// step's outcome: oracle/pbn_oracle.c's ext64, reset_draw, gap_of and step epilogue) is stated once,
// in step_law.h, the device statement of that law; the kernels here read and write memory around it.
// This file is the umbrella: the code lives in the pieces below, one per kernel (DESIGN.md
// "Refactoring the step kernels": a change that moves code between them is checked with
// tools/listing_diff.py).
#pragma once
#include "step_args.h"     // StepArgs, PolicyArgs
#include "step_debug.h"    // stamps, listing marks, checked indexing, StepRows
#include "step_parts.h"    // helpers of more than one kernel
#include "step_wave.h"     // pbn_step_wave
#include "rollout_pipe.h"  // pbn_rollout_pipe
#include "rollout_settle.h"  // pbn_rollout_settle
#include "step_small.h"    // pbn_hist_kernel, pbn_reset_kernel, step_kernel_for
