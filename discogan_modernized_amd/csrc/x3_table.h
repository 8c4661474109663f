// Kernel-argument table of the conv weights of a flat parameter group, by 64 x 64 tiles of their [K][J] plane images (J = 16 C, KRSC):
// shared by x3_transpose_kernel (igemm_dma_x3.hip) and adam_step_x3t_kernel (optim.hip), which tile a group the same way.
#pragma once
#define DG_X3T_MAX 48
struct X3TransposeTable {
    int n;
    int tile0[DG_X3T_MAX + 1];      // first tile of weight i (prefix sums); tile0[n] = grid
    int K[DG_X3T_MAX], J[DG_X3T_MAX];
    long off[DG_X3T_MAX];           // element offset of the weight inside a plane
};
