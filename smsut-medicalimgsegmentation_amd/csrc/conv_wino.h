// Internal interface between conv_mfma.hip (entry points, form selection) and conv_wino.hip (the large-reduction Winograd kernel).
#pragma once
#include "common.h"

// Shapes the kernel takes: 3x3 stride-1 "same", Kdim % 16 == 0 (>= 32), Ndim % 16 == 0, H % 16 == 0, W % 16 == 0.
bool smsut_wino_l_eligible(int N, int H, int W, int Kdim, int Ndim);

// One launch of conv_wino_l, described by a ConvCall (common.h; fp32 tensors only).  x2: the virtual cat([x, x2]); with sc->w and
// transposed_w it is the fused shortcut data-gradient instead (second half = the shortcut's gradient, 1x1 weights sc->w).  sc
// (forward): fused 1x1 shortcut conv.  wu: the caller's prepared image of w for THIS form (smsut_wino_prepare with the same Kdim,
// Ndim and transposed_w) or null = transform the weights on the fly; the library keeps no table of images (r03 did: SURVEY 8b rules
// process-wide mutable state out).  fin (statistics / BST forms): the InstanceNorm statistics are finalised inside the launch by the
// last-arriving workgroup.  Returns 0 when launched (or reported to tiles_out), -1 when the form is not covered (nothing launched).
int smsut_wino_l_launch(const ConvCall& c);
