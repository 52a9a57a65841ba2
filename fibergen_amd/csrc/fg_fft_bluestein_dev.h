// Launchers of the Bluestein tile kernels (fg_fft_bluestein.hip); fg_fft.hip calls them with the plans and tables Fft3 made.
#pragma once
#include "fg_fft_bluestein.h"
#include "fg_fft_smooth_dev.h"

namespace fg {
namespace fft {

void launch_bluestein_strided(const BluesteinArgs& a0, int nouter, int ncomp, long cs, hipStream_t s);
void launch_bluestein_z(const BluesteinZArgs& a, int ncomp, long comp_stride, hipStream_t s);

}  // namespace fft
}  // namespace fg
