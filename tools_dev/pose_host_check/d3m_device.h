// A stand-in for csrc/d3m_device.h, which csrc/d3m_set_sums.h includes: the wave_sum it needs is the stand-in d3m_aux.h's.
#pragma once
#include "d3m_aux.h"
float __shfl_xor(float v, int lane_mask, int width);        // named by WaveTree::XorButterfly only, which the pose does not use
