// The two properties of sigmoid_acc that best_class_cut (yolort_amd/csrc/post_common.hpp) relies on, swept on the CPU.  Built by tests/test_best_class.py against the
// simulator's header (tests/hipsim/hipsim.h: the kernel sources compile unchanged as host C++), so the functions under test are the ones the kernels call.
//   (A1)  x <= y                                              =>  f(x) <= f(y) * (1 + 2^-21)
//   (A2)  y in [BEST_VLOW, BEST_VCAP],  x < fl(y - BEST_DELTA)  =>  f(x) <= f(y) * (1 - 2^-19)
// Both are statements about the running maximum M(t) = max f(x) over x < t, so one ascending sweep with a trailing pointer checks them for EVERY pair.  Visited: every fp32
// value with 2^-12 <= |x| < 128 on the negative side and < 32 on the positive side (f is exactly 0 below -104 and exactly 1 above 17.4; every logit best_class_cut lets a
// cut depend on lies in [-30 - 2^-6, 8]), and 1024 evenly spaced mantissas of every other binade, the subnormals, both zeros and both infinities.
// Prints the worst figures; exit status 1 if a property fails.
#include "hipsim.h"
#include "post_common.hpp"

using namespace ymi;

static inline uint32_t key_of(float x) {   // ascending keys == ascending floats (-0 just below +0)
    const uint32_t b = __float_as_uint(x);
    return (b & 0x80000000u) ? ~b : (b | 0x80000000u);
}
static inline float float_of(uint32_t k) { return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k); }

static inline bool dense(float x) {
    const float m = fabsf(x);
    return m >= 0x1p-12f && (x < 0 ? m < 128.0f : m < 32.0f);
}
// the next visited key after k (k itself is visited)
static inline uint64_t next_key(uint64_t k) {
    const float x = float_of((uint32_t)k);
    if (dense(x)) return k + 1;
    const uint64_t n = (k | 0x1fffu) + 1;   // sparse: multiples of 2^13 in key space == 1024 mantissas per binade
    // never jump over the start of a dense stretch
    const uint32_t starts[4] = {key_of(-128.0f) + 1, key_of(0x1p-12f), key_of(-0x1p-12f) + 1, key_of(32.0f)};
    uint64_t best = n;
    for (uint32_t s : starts)
        if (s > k && s < best && dense(float_of(s))) best = s;
    return best;
}

int main() {
    const uint64_t k_begin = key_of(-INFINITY), k_end = key_of(INFINITY);
    double worst_a1 = 0.0, least_a2 = 1.0;
    float at_a1 = 0.f, at_a2 = 0.f;
    float m_all = 0.0f;                    // max f over every visited x < y
    float m_trail = 0.0f;                  // max f over every visited x < fl(y - BEST_DELTA)
    uint64_t kt = k_begin;                 // the trailing pointer
    long visited = 0, in_a2 = 0;
    bool bad = false;
    for (uint64_t k = k_begin; k <= k_end; k = next_key(k)) {
        const float y = float_of((uint32_t)k);
        const float fy = sigmoid_acc(y);
        ++visited;
        if (!(fy >= 0.0f && fy <= 1.0f)) { printf("f(%a) = %a out of range\n", y, fy); bad = true; }
        if (m_all > fy) {                  // (A1)
            const double ex = fy > 0.0f ? (double)m_all / (double)fy - 1.0 : INFINITY;
            if (ex > worst_a1) { worst_a1 = ex; at_a1 = y; }
        }
        if (y >= BEST_VLOW && y <= BEST_VCAP) {   // (A2)
            const float cut = best_class_cut(y, 1.0f);
            if (cut != __fsub_rn(y, BEST_DELTA)) { printf("best_class_cut(%a) = %a\n", y, cut); bad = true; }
            const uint64_t kc = key_of(cut);
            for (; kt < kc; kt = next_key(kt)) {
                const float ft = sigmoid_acc(float_of((uint32_t)kt));
                if (ft > m_trail) m_trail = ft;
            }
            const double gap = 1.0 - (double)m_trail / (double)fy;
            if (gap < least_a2) { least_a2 = gap; at_a2 = y; }
            ++in_a2;
        }
        if (fy > m_all) m_all = fy;
    }
    // what the cut does outside its conditions: nothing is filtered; above the cap: the cap
    if (best_class_cut(-30.5f, 1.0f) != -INFINITY || best_class_cut(0.0f, 0x1p-61f) != -INFINITY || best_class_cut(-INFINITY, 1.0f) != -INFINITY ||
        best_class_cut(NAN, 1.0f) != -INFINITY || best_class_cut(0.0f, NAN) != -INFINITY) { printf("the cut filters outside its conditions\n"); bad = true; }
    if (best_class_cut(24.0f, 0.5f) != BEST_VCAP - BEST_DELTA || best_class_cut(INFINITY, 0.5f) != BEST_VCAP - BEST_DELTA) { printf("the cut rises above the cap\n"); bad = true; }
    if (sigmoid_acc(BEST_VLOW) < 0x1p-44f || BEST_OMIN != 0x1p-60f) { printf("the product of the largest logit is not a normal number\n"); bad = true; }
    printf("visited %ld logits (%ld under A2)\n", visited, in_a2);
    printf("A1 worst fall of the running maximum: %.3g at %a (allowed %.3g)\n", worst_a1, at_a1, 0x1p-21);
    printf("A2 least step below the cut: %.3g at %a (required %.3g)\n", least_a2, at_a2, 0x1p-19);
    if (worst_a1 > 0x1p-21 || least_a2 < 0x1p-19) bad = true;
    printf(bad ? "FAILED\n" : "OK\n");
    return bad ? 1 : 0;
}
