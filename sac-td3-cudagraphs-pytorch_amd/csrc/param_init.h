// What engine.hip knows of the parameter initialiser (param_init.hip, param_init_kernels.h; include/sactd3_init.h is its C ABI): the
// argument structs and one host launcher per kernel.  Nothing else crosses between the two translation units.
#pragma once
#include <hip/hip_runtime.h>

#define PI_MAX_MATS 9        // actor layers 0 .. 2, critic net n layer l: 3 + 3 n + l
#define PI_MAX_SHORT 256     // min(rows, cols) of a weight: the hidden width, or a head narrower than it
#define PI_MAX_TALL 8192     // max(rows, cols): one column of G lives in LDS while it is orthogonalised
#define PI_MAX_REDRAW 8      // redraws of one column before it is given up (left zero, and counted once more)

// One weight matrix [rows, cols] at dst (row stride ld >= cols; the pad columns are written 0).  Its Gaussian G is
// [max(rows, cols), min(rows, cols)] at scratch + scratch_off, row-major: element e = i * min(rows, cols) + j.
struct InitMat { float* dst; int ld, rows, cols, id; long scratch_off; };
struct InitOrthArgs {
  InitMat m[PI_MAX_MATS]; int n;              // one workgroup per entry
  unsigned long long seed; unsigned epoch;    // the Philox key and the first counter word
  float* scratch;
  int* redrawn;                               // one device word: columns redrawn so far
};
// One family of nets (the actor; the twin critics): `nets` blocks of `size` floats, every offset a multiple of 4.  Weights are
// [0, b1), [W2, b2), [Wh, bh); the LayerNorm weights are [g1, g1 + 256) and [g2, g2 + 256); everything else is a bias or padding.
struct InitFanFam { float *P, *T, *T2, *T3, *M, *V; int nets, size, b1, g1, W2, b2, g2, Wh, bh; int* t; double* pw; };
struct InitFanArgs {
  InitFanFam f[2]; int nf;
  float* la; float la0; int* t_l; double* pw_l;      // la != NULL: the temperature's {log alpha, m, v} and its optimiser's words
};

// hipErrorInvalidValue, and nothing is launched, where an argument is outside what the kernel's tables hold; otherwise
// hipGetLastError() behind the launch.
hipError_t param_init_orth_launch(const InitOrthArgs& args, hipStream_t stream);
hipError_t param_init_fanout_launch(const InitFanArgs& args, hipStream_t stream);
