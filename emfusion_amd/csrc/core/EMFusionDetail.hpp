// EMFusionDetail.hpp -- helpers shared by the translation units of emf::EMFusion (not installed).
#pragma once

#include <cstdio>
#include <initializer_list>

#include "EMFusion.hpp"

namespace emf {
namespace detail {

enum Stamp { kStart = 0, kPoints, kEstep, kRaycast, kComposite, kIntegrate, kMasks, kNumStamps };

inline emf_pose_t toPose(const Affine3f& a) {
    emf_pose_t p;
    for (int i = 0; i < 9; ++i) p.R[i] = a.rotation().val[i];
    for (int i = 0; i < 3; ++i) p.t[i] = a.translation().val[i];
    return p;
}

// the fields of a line of absorbed.txt / lifted.txt, each after a blank: voxel triples, counts, floats in %.9g
inline void printInts(std::FILE* file, const int32_t (&v)[3]) {
    for (const int32_t x : v) std::fprintf(file, " %d", x);
}
inline void printCounts(std::FILE* file, std::initializer_list<uint64_t> counts) {
    for (const uint64_t v : counts) std::fprintf(file, " %llu", static_cast<unsigned long long>(v));
}
template <size_t N>
inline void printFloats(std::FILE* file, const float (&v)[N]) {
    for (const float x : v) std::fprintf(file, " %.9g", static_cast<double>(x));
}

}  // namespace detail
}  // namespace emf
