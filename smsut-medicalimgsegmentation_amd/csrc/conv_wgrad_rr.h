// Internal interface between conv_mfma_wgrad.hip (entry points, wgrad_select) and conv_wgrad_rr.hip (the register-row weight gradient).
#pragma once
#include "common.h"

// 3x3 stride-1 "same" weight gradient, slabs written per split as [split][9 (+1 with gs)][Cin][Cout] (the layout sum_splits reads).
// Shapes: W % 16 == 0, H % 4 == 0, Cin % 16 == 0, Cout % 16 == 0, 32-bit element offsets.  The cat form of a shape is eligible when
// a valid seam exists (ca % 16 == 0, 0 < ca < Cin: Cin >= 32); the call's own ca is checked by the launch.
// Number of split slabs the launch writes; 0 = not eligible.
int smsut_wgrad_rr_splits(const WgradKey& k);
// Returns 0 when launched, -1 when not covered (nothing launched).  c.b (nullable): PAIRED launch, see WgradSetB.
int smsut_wgrad_rr_launch(const WgradCall& c);
