// shapes.hpp -- the numbers on which the prune's kernels and the host's grid arithmetic (pass_plan.hpp) must agree: rows and columns of the
// work items of every pair kernel, the limits that choose between them, and the -D overrides that go with them.  Constants only: no kernel,
// no HIP call, so the CPU probes of the sizing functions compile this and none of the kernels.
#pragma once

constexpr int TILE_ROWS = 16;
constexpr int MAX_HP = 32;  // register-tiled kernel only; the sieve kernel takes any h

enum { ALGO_AUTO = 0, ALGO_TILE = 1, ALGO_SIEVE = 2, ALGO_LOCAL = 3 /* reported only: a pass run by the chunk-local kernel */ };

namespace tsc {

// ---- the chunk-local kernel (local_pass.hpp) ----
constexpr int LP_MAX_ROWS = 2048;  // longest chunk (structures) the chunk-local kernel takes
constexpr int LP_TI = 16;                       // rows per work item
#ifndef TSC_LP_TPB
#define TSC_LP_TPB 4
#endif
// row tiles one block is sized for: one per wavefront (measured against two: a wavefront walks its tiles one after the other, and
// a pass of this kernel is as long as its slowest wavefront -- C3's k = 500 pass 44 -> 39 us, a 20 000-structure call 0.71 -> 0.64 ms)
constexpr int LP_TILES_PER_BLOCK = TSC_LP_TPB;

// ---- the culled pass (cull.hpp, cull_mm.hpp) ----
constexpr int CULL_MAX_CHUNKS = 64;                         // passes with more chunks are not culled (their chunks are short anyway)
constexpr int CULL_COLS = 128;                              // columns per tile (the pair kernel's CPL = 2)
#ifndef TSC_CULL_XCD_RUN
#define TSC_CULL_XCD_RUN 32
#endif
constexpr int CULL_XCD_RUN = TSC_CULL_XCD_RUN;              // option "cull_xcd": consecutive row groups (of 4 tiles) that stay on one XCD
constexpr int CMM_SEG = 1024;             // columns per work item (queue entries keep the column offset in 10 bits)

// ---- the screen on the matrix cores (mm.hpp) ----
constexpr int MM_ROWS = 64;                 // rows per work item
constexpr int MM_STEP = 16;                 // columns per step
#ifndef TSC_MM_LEVEL2
#define TSC_MM_LEVEL2 0   // 1: level 2 (mm.hpp) where a pair is decoded in the 64-row kernels.  Measured at C4: 6.95 ms with it, 6.74 without -- the 7 %
                          // more pairs that reach H cost less than its eight loads in front of every batch; the 16-row kernel never had it
#endif
#ifndef TSC_MM_WAVES
#define TSC_MM_WAVES 4
#endif
constexpr int MM_WAVES = TSC_MM_WAVES;   // wavefronts (work items) per workgroup of the walked passes' kernel
// work items (wavefronts) per workgroup of the 16-row kernel: 2 where most workgroups of the grid have work (a workgroup keeps its slot until
// its longest item is through: C3's k = 100 .. 2 passes 2 - 4 us shorter than with 4), 4 where most are empty and the launch is its dispatch
// (C3's last pass: 28 us against 44) -- the host picks by the columns a row of the pass can have: more than MM16_LONG_SEGS segments of 512
// (pass_plan.hpp: mm16_items_per_workgroup)
constexpr int MM16_LONG_SEGS = 64;

}  // namespace tsc
