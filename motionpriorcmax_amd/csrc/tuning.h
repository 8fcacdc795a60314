// Compile-time constants of libmpcmax that a tuning sweep may override (tools/sweep_*.sh, tools/ab_*.sh set MPC_EXTRA_HIPCC_FLAGS=-DNAME=value;
// never set for a product build): every one with the measurement that chose its value.  Collected here (round 5) so that the
// translation units read as product code; the values are the ones the kernels were profiled with.
#pragma once

// ---- contrast.hip --------------------------------------------------------------------------------------------------
#ifndef CM_PF
#define CM_PF 4      // rows of the raw image in flight ahead of the row being processed (2: 35.5 us at C3, 4: 34.7, 8: 34.3)
#endif
#ifndef MPC_SM_PF
#define MPC_SM_PF 2
#endif

#ifndef MPC_CS_ORDER
#define MPC_CS_ORDER 0    // k_contrast_smooth_march: order of the two kinds of workgroup in the 1-D grid.  0: contrast first, 1: smoothness
                          // first, 2: interleaved in proportion to their counts.  Launch time in us (HIP events, inside the step, two
                          // runs of 20 steps each) against k_contrast_march + k_lut_smooth_march in launches of their own:
                          //          two launches    0             1             2             2, eight at a turn
                          //   C3     33.6 + 23.6     46.7 / 47.1   46.6 / 46.8   54.1 / 54.1   53.2 / 53.7
                          //   C2     11.7 +  8.1     12.0 / 12.1   12.7 / 12.9   13.2 / 13.1   12.7 / 13.0
                          //   C4     11.6 + 10.4     12.4 / 12.3   14.2 / 14.1   13.8 / 14.2   13.8 / 13.8
                          // Every order beats the two launches at all three sizes, so there is no size below which mpc_focus_fwd goes
                          // back to them (profiles/contrast_smooth_runs.md)
#endif

// ---- events.hip ----------------------------------------------------------------------------------------------------
#ifndef EV_PER_THREAD
#define EV_PER_THREAD 2   // measured at C3: 2 -> 98.6 us, 4 -> 106.9, 8 -> 107.5 (whole forward splat)
#endif
#ifndef EV_STAGE
#define EV_STAGE 1152      // records of one workgroup laid out in LDS before they are written (>= 2.25 per event)
#endif
#ifndef EV_LUT_THREADS
#define EV_LUT_THREADS 512
#endif
#ifndef EV_LUT_MINWAVES
#define EV_LUT_MINWAVES 6    // wavefronts per SIMD the register budget of k_lut_accum<false> is set for: 6 = three 512-thread workgroups per CU (what
                             // its 46 KB LDS strips are sized for); the kernel had drifted to 81 VGPRs -- one over the 80 of six wavefronts, i.e. TWO
                             // workgroups per CU (round 6, see profiles/HISTORY_r06.md)
#endif
#ifndef EV_LUT_THREADS_ORD
#define EV_LUT_THREADS_ORD 1024      // ordered variant: 72 KB of LDS per workgroup -> two per CU; 1024 threads keep the CU's waves
#endif
#ifndef EV_LUT_INFLIGHT_ORD
#define EV_LUT_INFLIGHT_ORD 2
#endif
#ifndef EV_LUT_INFLIGHT
#define EV_LUT_INFLIGHT 4   // records of a thread in flight together.  Round 3, stage call: 4: 43.8 us, 5: 42.4, 6: 43.6, 8: 52.3; round 6, inside the step and at
                            // three workgroups per CU (EV_LUT_MINWAVES): 4: 55.9 us at C3 / 44.7 at C4 batch 6, 5: 56.9 / 45.7, 6: 63.0 / 51.2
#endif

#ifndef EV_LUT_ADD_PF
#define EV_LUT_ADD_PF 6     // k_lut_accum<false>: cells of add_term a thread requests at the top of the kernel, with the records (12 VGPRs); 6 x 512
                            // threads cover the 2 880 cells of a C3 strip, the cells beyond are read where they are used.  k_lut_accum<false>,
                            // rocprofv3 averages: 0: 47.2 us at C3 / 40.3 at C4 batch 6, 6: 44.1 / 39.9 (parent 53.1 / 45.4)
#endif

// ---- knn.hip -------------------------------------------------------------------------------------------------------
#ifndef KNN_BW_CH
#define KNN_BW_CH 4       // bwd_window_fast: cells of a window row whose LDS reads are issued together
#endif
#ifndef KNN_BW_PITCH
#define KNN_BW_PITCH 48   // row pitch (cells) of the staged arrays without the flow_to_next gradient; >= 16 + 2 * KNN_RQ_MAX
#endif
#ifndef KNN_BW_PITCH_NEXT
#define KNN_BW_PITCH_NEXT 32   // ... with the flow_to_next gradient (20 bytes per cell)
#endif
#ifndef KNN_BW_OCC
#define KNN_BW_OCC 7
#endif
#ifndef KNN_BW_OCC_IWD
#define KNN_BW_OCC_IWD 7      // 'iwd' without the flow_to_next gradient (12 bytes of LDS per cell as for 'mean'): k_knn_bwd_tile at C3 155.1 us at six per CU, 148.6 at seven
#endif
#ifndef KNN_BW_OCC_NEXT
#define KNN_BW_OCC_NEXT 6     // with the flow_to_next gradient (and for 'iwd'): 80 VGPRs, 23 KB of LDS per workgroup.  C4 batch 6, k_knn_bwd_tile:
                              // 8 per CU by registers (64, 31 spilled; the LDS -- 24 bytes per cell then -- allowed 5) 242 us; the K-th index
                              // out of the LDS (20 bytes per cell: 6 per CU) at 8 / 6 / 5: 218 / 206 / 215; + the conflict-free pitch where the
                              // region leaves room (k_knn_bwd_tile: RP) at 7 / 6 / 5: 209 / 202 / 212  (profiles/r06_ab_bwd_next.txt)
#endif
#ifndef KNN_FAR_QB
#define KNN_FAR_QB 256        // far queries tested against the tile per batch (one per thread); those that touch it: a list in LDS
                              // (512 / 1024 per batch: 244 / 273 us against 237 at a 48 px contraction band)
#endif
#ifndef KNN_FAR_BLOCKS
#define KNN_FAR_BLOCKS 4096     // (2048: 237 us against 218 at a 48 px contraction band)
#endif

#ifndef KNN_BW_PRIO
#define KNN_BW_PRIO 0         // k_knn_bwd_tile: issue priority (MPC_PRIO) of its phases.  0: none, the kernel as it was; 1: raised from entry to the window
                              // loop (reach, row ranges, staging), 0 in the loop; 2: as 1 and raised again for the final stores.
                              // Measured, not kept (profiles/issue_prio_runs.md): the phase before the loop falls from 4.5 to 2.9 us of a workgroup and
                              // the loop grows by as much -- lifetime 10.3 -> 10.4 us; k_knn_bwd_tile at C3, kernel trace, medians of two runs each:
                              // 0: 106.9 / 104.9 us, 1: 106.5 / 105.4, 2: 108.2 / 106.4 (2 also spills three more registers with flow_to_next + 'iwd')
#endif

// ---- knn_strip.hip -------------------------------------------------------------------------------------------------
#ifndef KS_PRIO
#define KS_PRIO 1                   // k_knn_strip (main launch only; the tail's strip workgroups run with few waves per SIMD): issue priority (MPC_PRIO)
                                    // of its phases.  0: none, the kernel as it was; 1: raised from the start of the body to the "staged" barrier, 0 from
                                    // pass 1 on; 2: priority 2 up to that barrier, 0 from pass 1 through the ranking of the K-th level, 1 from the outputs on.
                                    // k_knn_strip at C3, kernel trace, medians of two runs each (profiles/issue_prio_runs.md): 0: 214.6 / 215.9 us,
                                    // 1: 204.5 / 205.5; in the visit before, with 2 beside them: 0: 222.1 / 215.1, 1: 210.9 / 205.3, 2: 211.7 / 205.7.
                                    // A workgroup's phases (white noise): before the search 11.4 -> 7.4 us, search 8.7 -> 11.9, lifetime 20.1 -> 19.3:
                                    // most of what the load phases gain the search gives back, the rest is the 10 us.  2 buys nothing over 1.
#endif
#ifndef KS_MORE_MIN
#define KS_MORE_MIN 16               // a strip becomes a far item of the tail launch for its unfinished queries if it has more than this many (or far queries)
#endif
#ifndef KS_MAIN_CHORD
#define KS_MAIN_CHORD 1            // main launch: region rows as wide as the widest chord (1) or square (0) that uses them
#endif
#ifndef KS_MAXCH_FAR
#define KS_MAXCH_FAR 48             // ... of a far item of the tail launch (192 slots: a band along the left or right border -- every region row
                                   // as wide as the widest chord -- needs ~160; 256 slots at three workgroups per CU measured slower, see KS_MORE_OCC)
#endif
#ifndef KS_SB
#define KS_SB 3                     // staging: items per thread whose global loads are in flight together
#endif
#ifndef KS_FORWARD_MAX
#define KS_FORWARD_MAX 1024         // the main launch marked at most this many queries: the tail's fallback workgroups take them from the marked list, no far items
#endif
#ifndef KS_MORE_OCC
#define KS_MORE_OCC 4               // workgroups per CU of the tail launch (k_knn_tail) = its register budget (128; 13 registers spill).  The launch is bound
                                   // by the latency of its work items: C3, 40 px translation / 48 px contraction band: 4 per CU with 192 slots
                                   // 161 / 308 us, 3 per CU with 192 slots 179 / 351, with 256 slots 190 / 368, 2 per CU 258 / -
#endif

// ---- voxel.hip -----------------------------------------------------------------------------------------------------
#ifndef VOX_STRIP_KB
#define VOX_STRIP_KB 75       // LDS budget of a strip: two workgroups per CU, whose zero / accumulate / write phases overlap (150 KB, one per CU:
                              // 0.283 ms against 0.265 at the DSEC batch shape; 50 KB: the binning pass pays for the extra buckets)
#endif

// ---- repr.hip ------------------------------------------------------------------------------------------------------
#ifndef REPR_STRIP_KB
#define REPR_STRIP_KB 75      // LDS budget of a strip of the centred voxel grid (the input rows behind a range of output rows): the fastest of
                              // 37 / 50 / 75 / 150 KB for the whole call at the C4 batch (6 x 65 x 480 x 640 -> 384 x 512; two workgroups per CU at 75,
                              // one at 150): tools/repr_call_time.py under one build each, figures in DESIGN.md 7 f-2b
#endif

// ---- common.h ------------------------------------------------------------------------------------------------------
#ifndef MPC_CT_H
#define MPC_CT_H 32
#endif

// ---- knn_device.h --------------------------------------------------------------------------------------------------
#ifndef KNN_BINS
#define KNN_BINS 32
#endif
#ifndef KNN_BATCH
#define KNN_BATCH 2   // candidate positions loaded ahead of use in the two hot scans (B=14: 944 -> 874 us; 4: 867)
#endif
#ifndef KNN_RCAP
#define KNN_RCAP 6                 // largest search radius (cells) of the strip kernel's main launch
#endif
#ifndef KNN_FAR_RINGS
#define KNN_FAR_RINGS 2            // a K-th distance beyond r_init + this many rings: the far backward's query (knn_is_far_dk)
#endif

