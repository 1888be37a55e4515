// pgbart_hip.hip -- particle-Gibbs BART for MI355X (gfx950 / CDNA4), C ABI of include/pgbart.h.
//
// Replaces the native sampler the reference imports from the external `bartrs` wheel
// (pymc_bart/pymc_bart.py:2; call site tests/test_bart.py:231-235).  Algorithm: SURVEY.md
// Appendix A (upstream PGBART.astep) under the numeric contract of include/pgbart_spec.h.
//
// Design:
//   * The whole astep is a DEVICE-RESIDENT STATE MACHINE.  The host only enqueues identical
//     "slots" = { k_ctrl ; k_rows [; k_loglik] } on one HIP stream and polls a pinned progress
//     word; it never waits for the device inside a tree update.  k_ctrl (one 256-thread
//     workgroup per particle) finishes the previous SMC round from the integer statistics the
//     row pass produced -- leaf values, particle weights, systematic resampling on one wave, the
//     next growth proposal incl. the exact "k-th row of the leaf" selection -- and writes one
//     job per particle.  k_rows streams the rows on a persistent grid: a work item is a 1024-row
//     chunk times a group of particles with work; it relabels the rows of the leaves being split
//     and reduces the children's sufficient statistics (four values per butterfly, wave_sum4).
//     The slot that starts a tree fuses FINAL(previous tree) + INIT + round 0 into one pass.
//   * HBM layout: X column-major (coalesced column streams), {sum_trees, residual} packed as
//     double2 per row, one BYTE leaf label per row per particle in an 8-generation ring (idle
//     particles are never copied; a pass writes only particles that split).
//   * All row reductions are integer (fixed point) => bit-reproducible, independent of
//     launch geometry and atomics order, and identical to the CPU oracle.
//   * Kernel instances are compiled per data set where the hot loop has no registers or
//     instructions to spare: k_rows<SubsetSplit columns?, Normal family?, linear response?>,
//     k_rows_mk<K>, k_loglik<K, family>, k_ctrl<multi-output?, linear response?, order keys?>.
//   * No MFMA: the path is gather / partition / reduce (HBM / L2 bound).
//
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <hipcub/hipcub.hpp>  // (device radix sort: the order keys of the design matrix, pgb_set_data)

#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <atomic>
#include <chrono>
#include <mutex>
#include <sched.h>
#include <thread>
#include <type_traits>
#include <vector>

#include "pgbart.h"
#include "pgbart_image.h"
#include "pgbart_pack.h"
#include "pgbart_spec.h"
#include "pgbart_compiled.h"  // (family 11: its code object is compiled at run time, k_loglik_compiled.hip)
#include "pgbart_logpdf.h"
#include "pgbart_pointwise.h"
#include "pgbart_psis.h"
#include "pgbart_ice.h"
#include "pgbart_rowsummary.h"
#include "pgbart_score.h"
#include "pgbart_rowreduce.h"
#include "pgbart_proximity.h"
#include "pgbart_diag.h"
#include "pgbart_ppc.h"
#include "pgbart_shap.h"
#include "pgbart_permimp.h"
#include "pgbart_ale.h"
#include "pgbart_hstat.h"
#include "pgbart_arms.h"
#include "pgbart_surv.h"
#include "pgbart_rank.h"

#include "pgb_dims.h"

// One translation unit; the parts below are included in this order (each relies on the ones above).
#include "pgb_dev_types.h"
#include "pgb_dev_helpers.h"
#include "pgb_leaf_values.h"
#include "k_ctrl.h"
#include "k_rows.h"
#include "k_rows_mk.h"
#include "k_loglik.h"
#include "pgb_pred_walk.h"
#include "k_setup_predict.h"
#include "k_pointwise.h"
#include "k_export.h"
#include "pgb_host.h"
#include "pgb_pred_host.h"
#include "pgb_checkpoint.h"
#include "pgb_probe.h"
#include "pgb_pointwise_host.h"
#include "k_psis.h"
#include "k_ice.h"
#include "k_rowsummary.h"
#include "k_rowscore.h"
#include "k_diag.h"
#include "k_ppc.h"
#include "pgb_ppc_compiled_host.h"
#include "k_pdp.h"
#include "k_shap.h"
#include "k_shap_interaction.h"
#include "k_rowreduce.h"
#include "k_proximity.h"
#include "k_permimp.h"
#include "k_ale.h"
#include "k_hstat.h"
#include "k_arms.h"
#include "k_surv.h"
#include "k_rank.h"
