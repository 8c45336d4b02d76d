// One MLP of the engine as the side units' kernels read it (dormant.hip: the scan, the recycler and the feature rank; action_values.hip:
// candidate scoring).  engine.hip fills it in one place (net_view) and sees nothing else of hidden_tile.h, whose ring front end reads it.
#pragma once

#define HT_HID 256         // width of both hidden layers
#define HT_TILE 16         // rows of one tile: the 16 rows of v_mfma_f32_16x16x4f32 (the launchers cut their grids by it)

// P: the net's parameter block; the NetLayout offsets in floats inside it (W [out][in], row-major, W1 with row stride ld1); K the input
// width (a ring record's leading K floats); nh the head's rows.  M / V: Adam's exp_avg / exp_avg_sq of the same block, NULL where no kernel
// writes parameters (the recycler alone does).  id: 0 the actor, 1 / 2 the critics.
struct NetView {
  float *P, *M, *V;
  int id, K, ld1, nh;
  int W1, b1, g1, be1, W2, b2, g2, be2, Wh;
};
