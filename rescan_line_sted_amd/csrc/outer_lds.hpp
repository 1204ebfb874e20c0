// outer_lds.hpp -- LDS byte counts of the outer-decimation column kernels (conv_kernels.hpp colconv_outer_body, geometry
// in fft_configs.hpp OuterCol<L>).  One definition for the launcher (fft_kernels.hip launch_col / prepare) and for the host
// emulator (tests/emu/long_outer_emu.cpp), which allocates exactly what the launcher pays for.
#pragma once
#include <cstddef>
#include "conv_kernels.hpp"
#include "fft_configs.hpp"

namespace rl {

// complex LDS entries of the twiddle copy (conv_kernels.hpp colconv_outer_body TWLDS)
template <class OC>
constexpr size_t outer_tw_lds_elems(int twlds) {
    return (twlds > 0 ? PassTw<typename OC::Core, false, 0>::TOTAL : 0) + (twlds > 1 ? (OC::M - 1) * OC::Core::L : 0);
}
// the whole pass, f32: transform regions of CW columns + parking space + twiddle copies
template <class OC>
constexpr size_t outer_whole_lds_bytes() {
    return ((size_t)OC::CW * LdsSlots<typename OC::Core>::value + (size_t)OC::PARK * 64 * OC::CW + outer_tw_lds_elems<OC>(OC::TWLDS)) * sizeof(cx<float>);
}
// the whole pass, float64: C64 columns, PARK64 parked values per lane, no twiddle copies
template <class OC>
constexpr size_t outer_whole_lds_bytes_f64() {
    return ((size_t)OC::C64 * LdsSlots<typename OC::Core>::value + (size_t)OC::PARK64 * 64 * OC::C64) * sizeof(cx<double>);
}
// the halves of the split pass (f32): C columns + their twiddle copies
template <class OC>
constexpr size_t outer_split_lds_bytes() {
    return ((size_t)OC::C * LdsSlots<typename OC::Core>::value + outer_tw_lds_elems<OC>(OC::TWLDS_SPLIT)) * sizeof(cx<float>);
}
// ... of the kernel of one type and mode (float64: the whole pass only)
template <class OC, typename T, int MODE>
constexpr size_t outer_lds_bytes() {
    if constexpr (sizeof(T) != 4) return outer_whole_lds_bytes_f64<OC>();
    else if constexpr (MODE == COL_PER_IMAGE) return outer_whole_lds_bytes<OC>();
    else return outer_split_lds_bytes<OC>();
}

}  // namespace rl
