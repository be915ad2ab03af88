// gbp_kernels.hip — CDNA4 (gfx950) kernels of one synchronous GBP iteration: THE device translation unit of the library.
//
// This file is a map.  The code lives in the units under kernels/, each of which names what it uses by #include; they are
// compiled HERE, as one translation unit, so every library holds one gfx950 code object (loaded once, in gbp_create).
//
// Replaces the reference's per-iteration Poplar program (ba/ba.cpp:895-905):
//   kernels/gbp_sweep.hip      k_sweep        PrepMessageVertex + Copy(mu,oldmu) + the four Compute*Message*Vertex classes
//                                             (gbp_codelets.cpp:215-710) + the camera half of popops::reduceWithOutput
//                                             (ba.cpp:129-132) as per-row partial sums + Copy(msg,pmsg) (in-place messages)
//                              k_linearise    RelineariseFactorVertex (gbp_codelets.cpp:20-172)
//                                             + WeakenPriorVertex (gbp_codelets.cpp:176-197) inside the refresh WEAKEN_PRIORS ends with
//   kernels/gbp_beliefs.hip    k_beliefs*     the rest of buildUpdateBeliefsProg (ba.cpp:104-139): camera rows + prior, landmark messages
//                                             + prior; k_gather_peers / k_gather_slices of the peer-memory exchanges
//   kernels/gbp_persist.hip    k_persist_flow n iterations of the two above inside ONE launch (graphs whose workgroups are all resident
//                                             at once), hand-offs through tagged records; k_persist_probe, persist_grid, launch_persist.
//                                             (k_persist, the barrier kernel it replaced: hooks/gbp_persist_barrier.hip, test-hooks builds only)
//   kernels/gbp_metric.hip     k_means/k_eval eval_reprojection_error (util.cpp:74-144) + counters (ba.cpp:1011-1020); k_eval_ride and the
//                                             device-side folds
//   kernels/gbp_state_io.hip   k_upload_* / k_read_state_dev / k_keyframe_state_dev / k_state_set / k_rec_copy / k_copy_segments:
//                                             WRITE / READ_PROG / NEW_KEYFRAME streams between the caller's arrays and the device records
// Every unit holds its kernels AND the launchers of exactly those kernels (gbp_kernels.h declares them).  Device helpers (GBP_DEV, no kernels):
//   kernels/gbp_tile.hpp             tile and record access: load_tile / store_tile, row16_sums_store, lmsg_tile_in / _out, the landmark quads
//   kernels/gbp_vertex.hpp           the vertex layer: belief means, relin_core, the camera-message records, factor_update
//   kernels/gbp_metric_math.hpp      the metric math: solve_pivot, eval_residual, the order of the metric's sums, ride_metric
//   kernels/gbp_persist_support.hpp  XwBuf, the counter barrier, persist_place, a tile wave's register state, the flow_* waits
//
// Mapping: one LANE per factor, 64 factors per wavefront, all blocks in VGPRs.
// The sweep is HBM-bound: every per-factor stream is a tile-coalesced 16-B-per-lane access, the
// 6x6/3x3 algebra (no MFMA: the blocks are tiny and chains are serial) hides under the loads.
// fp32 throughout, compiled with -ffp-contract=off so results are bit-comparable with the oracle.
#include "kernels/gbp_sweep.hip"
#include "kernels/gbp_beliefs.hip"
#include "kernels/gbp_persist.hip"
#include "kernels/gbp_state_io.hip"
#include "kernels/gbp_metric.hip"

#ifdef GBP_BUILD_TEST_HOOKS
#include "hooks/gbp_flow_torture.hip"        // k_flow_torture: the detector under the tagged records' untorn-16-byte-store assumption
#include "hooks/gbp_debug_vertex.hip"        // k_debug_vertex: relin_core / factor_update on caller-supplied factors (tests only)
#include "hooks/gbp_debug_math.hip"          // k_debug_math: the device math layer on caller-supplied vectors (tests only)
#endif
#ifdef GBP_BUILD_EXPERIMENTS
#include "experiments/gbp_lab_kernels.hip"   // mapping experiments and timing ablations (profiles/ only)
#endif
