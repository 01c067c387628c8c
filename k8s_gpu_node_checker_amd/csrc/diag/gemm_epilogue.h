// The LDS-patch epilogue of GEMM v3, v4 and v4's tail: how a wave empties its patch.  A wave owns a patch of 16 rows x
// NB * 16 fp32 columns (NB 16-column blocks: 4 in v3 and the tail, 8 in v4), fills it with one m-row of accumulator
// blocks and empties it in 16-byte row pieces.  The three kernels' C is compared bit for bit, so they take the walk's
// geometry from here.  Plain constexpr C++, no HIP: tests/test_gemm_epilogue_cpu.py compiles it with the host compiler.
#ifndef K8S_GPU_NODE_CHECKER_AMD_GEMM_EPILOGUE_H_
#define K8S_GPU_NODE_CHECKER_AMD_GEMM_EPILOGUE_H_

// Which piece of the patch a lane takes at step q: ELEMS fp32 elements (8 leave as bf16, 4 as fp32: 16 bytes either
// way) of row row(lane, q), from column col(lane) on.  One instruction of the wave covers RPI whole rows.
template <int NB, int ELEMS>
struct PatchWalk {
  static constexpr int LD = NB * 16 + 4;       // the patch's row stride in floats
  static constexpr int LPR = NB * 16 / ELEMS;  // lanes per row
  static constexpr int RPI = 64 / LPR;         // rows per instruction
  static constexpr int STEPS = 16 / RPI;
  static constexpr int row(int lane, int q) { return q * RPI + lane / LPR; }
  static constexpr int col(int lane) { return lane % LPR * ELEMS; }
};

#endif  // K8S_GPU_NODE_CHECKER_AMD_GEMM_EPILOGUE_H_
