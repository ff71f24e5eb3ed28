// Host-only helpers shared by every translation unit of libs2v (no HIP headers: the conv planner,
// conv_plan.cpp, compiles with a plain host compiler).
#pragma once
#include <cstdarg>
#include <cstdio>

#include "../../include/s2v.h"

namespace s2v {

void set_error(const char *fmt, ...);
int check_launch(const char *what);
int device_cus();
long long tune_get(int key);   // s2v_tune knobs (conv_plan.cpp)

#define S2V_REQUIRE(cond, ...)            \
    do {                                  \
        if (!(cond)) {                    \
            ::s2v::set_error(__VA_ARGS__);\
            return S2V_E_INVALID;         \
        }                                 \
    } while (0)

inline unsigned cdiv(long long a, long long b) { return (unsigned)((a + b - 1) / b); }

}  // namespace s2v
