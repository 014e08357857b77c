// launch_dispatch.h -- run-time bools into template arguments, for the launch glue of wavefront.hip and local_pool.hip.
#pragma once
#include <type_traits>

namespace rayrs {

// with_bools(f, a, b, ...) calls f(A, B, ...) where A is std::true_type{} or std::false_type{} as a is true or false, and so
// on: inside f, A() is a constant expression and may pick a kernel template's instance.  Every combination of the
// bools is instantiated, so the kernels a launch wrapper can start are the ones its lambda names, for all values.
template <class F> auto with_bools(F f) { return f(); }
template <class F, class... Rest>
auto with_bools(F f, bool b, Rest... rest) {
    return b ? with_bools([&](auto... cs) { return f(std::true_type{}, cs...); }, rest...)
             : with_bools([&](auto... cs) { return f(std::false_type{}, cs...); }, rest...);
}

}  // namespace rayrs
