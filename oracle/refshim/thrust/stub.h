/*
 * Stand-in for the thrust headers the reference's common header names.  TEST INFRASTRUCTURE ONLY.
 * Only what the exported entry points reach is real: the strided iterator over a matrix that
 * GpuMatBeginItr / GpuMatEndItr build, and exclusive_scan over it.  The algorithms behind the
 * functions that are not exported (count_if, copy_if, sort) abort when called.
 */
#pragma once
#include <cstdlib>
namespace thrust {
template <class A, class B> struct unary_function {};
template <class T> struct device_ptr { T* p; };
template <class T> struct counting_iterator { T v; };
template <class F, class I> struct transform_iterator { I it; F f; };
template <class E, class I> struct permutation_iterator { E e; I i; };
template <class T> device_ptr<T> device_pointer_cast(T* p) { return {p}; }
template <class T> counting_iterator<T> make_counting_iterator(T v) { return {v}; }
template <class I, class F> transform_iterator<F, I> make_transform_iterator(I i, F f) { return {i, f}; }
template <class E, class I> permutation_iterator<E, I> make_permutation_iterator(E e, I i) { return {e, i}; }

template <class T, class F>
using strided_it = permutation_iterator<device_ptr<T>, transform_iterator<F, counting_iterator<int>>>;
template <class T, class F> T& ref_at(const strided_it<T, F>& it, int k) { return it.e.p[it.i.f(it.i.it.v + k)]; }

/* out[k] = sum of in[0..k-1], in place allowed (reads in[k] before writing out[k]) */
template <class T, class F>
strided_it<T, F> exclusive_scan(strided_it<T, F> first, strided_it<T, F> last, strided_it<T, F> out) {
    const int n = last.i.it.v - first.i.it.v;
    T acc = 0;
    for (int k = 0; k < n; ++k) {
        const T v = ref_at(first, k);
        ref_at(out, k) = acc;
        acc += v;
    }
    return out;
}
template <class... A> int count_if(A&&...) { abort(); }
template <class... A> void copy_if(A&&...) { abort(); }
template <class... A> void sort(A&&...) { abort(); }
}
