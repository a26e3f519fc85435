// Runtime shape -> compile-time tags (host only).  Each dispatcher calls the
// generic callable once with one tag per axis.  An int / bool tag converts to
// its value in a constant expression; tag_t names the type of a dtype tag:
//   dispatch_th(dtype, hidden, [&](auto t, auto h) {
//       return launch<tag_t<decltype(t)>, h>(...);
//   });
// Every branch of one dispatcher returns the callable's one return type.
#pragma once

#include <type_traits>

#include "common.h"

namespace ml {

template <typename T> struct TypeTag { typedef T type; };
template <int V> using IntTag = std::integral_constant<int, V>;
template <typename Tag> using tag_t = typename Tag::type;

// mlearn_mlp_policy::dtype -> T (validate_policy admits bf16 and f32 only)
template <typename F> auto dispatch_dtype(int dtype, F&& f) {
    return dtype == MLEARN_DTYPE_BF16 ? f(TypeTag<bf16>{}) : f(TypeTag<float>{});
}

// hidden width -> H (validate_policy admits 64, 128 and 256 only)
template <typename F> auto dispatch_hidden(int hidden, F&& f) {
    switch (hidden) {
        case 64: return f(IntTag<64>{});
        case 128: return f(IntTag<128>{});
        default: return f(IntTag<256>{});
    }
}

// head columns (head_cols()) -> HC
template <typename F> auto dispatch_head(int hc, F&& f) {
    return hc == MLEARN_HEAD_COLS ? f(IntTag<MLEARN_HEAD_COLS>{}) : f(IntTag<MLEARN_HEAD_COLS_MAX>{});
}

template <typename F> auto dispatch_bool(bool b, F&& f) {
    return b ? f(std::true_type{}) : f(std::false_type{});
}

// num_layers -> L in 1..MLEARN_MAX_LAYERS
template <typename F> auto dispatch_layers(int L, F&& f) {
    static_assert(MLEARN_MAX_LAYERS == 4, "dispatch_layers lists the depths 1..4");
    switch (L) {
        case 1: return f(IntTag<1>{});
        case 2: return f(IntTag<2>{});
        case 3: return f(IntTag<3>{});
        default: return f(IntTag<4>{});
    }
}

// Projection slot counts with a kernel instantiation: 2 L (trunk kernels +
// LayerNorms, L <= MLEARN_MAX_LAYERS) and 2 L + 8 (the LSTM gate kernels).
constexpr int kMaxProjSlots = 16;

// projection slots -> NS in {2, 4, .., kMaxProjSlots}; miss() for any other count
template <typename F, typename G> int dispatch_slots(int nslot, F&& f, G&& miss) {
    static_assert(kMaxProjSlots == 16, "dispatch_slots lists the even counts 2..16");
    switch (nslot) {
        case 2: return f(IntTag<2>{});
        case 4: return f(IntTag<4>{});
        case 6: return f(IntTag<6>{});
        case 8: return f(IntTag<8>{});
        case 10: return f(IntTag<10>{});
        case 12: return f(IntTag<12>{});
        case 14: return f(IntTag<14>{});
        case 16: return f(IntTag<16>{});
        default: return miss();
    }
}

// (dtype, hidden) -> f(T, H): the minibatch launchers
template <typename F> auto dispatch_th(int dtype, int hidden, F&& f) {
    return dispatch_dtype(dtype, [&](auto t) {
        return dispatch_hidden(hidden, [&](auto h) { return f(t, h); });
    });
}

// (dtype, hidden, head columns, recurrent) -> f(T, H, HC, RNN): the policy kernels
template <typename F> auto dispatch_policy(int dtype, int hidden, int hc, bool rnn, F&& f) {
    return dispatch_th(dtype, hidden, [&](auto t, auto h) {
        return dispatch_head(hc, [&](auto c) {
            return dispatch_bool(rnn, [&](auto r) { return f(t, h, c, r); });
        });
    });
}

}  // namespace ml
