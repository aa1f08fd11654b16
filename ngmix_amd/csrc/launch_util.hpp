// launch_util.hpp -- host only: the one way a launcher starts a kernel.
//
// A launcher picks a Kernel{function, census name} -- from a constexpr table of
// rows searched linearly (find_kernel), or, where the instantiations are a product
// of template lists, with for_int<...> -- and hands it to launch(), which counts
// it in the census, opts in to large LDS, launches and reports the error.
#pragma once
#include <stdio.h>

#include <initializer_list>
#include <type_traits>
#include <utility>

#include "common.hpp"

namespace ngmix {

// a kernel instantiation and the name the launch census counts it under
// (name nullptr: a kernel no census test looks for; fn nullptr: no kernel --
// what find_kernel gives for keys outside its table, and launch() refuses)
template <typename... P>
struct Kernel {
    void (*fn)(P...);
    const char *name;
};

template <typename... P>
constexpr Kernel<P...> kernel(void (*fn)(P...), const char *name)
{
    return Kernel<P...>{fn, name};
}

// The census name of an instantiation whose template arguments come from a
// template product, "kernel<1, 2, 3>".  Held as a function-local static of the
// code that names the instantiation: formatted once, not per launch.
struct CensusName {
    char s[64];
    CensusName(const char *kern, std::initializer_list<int> args)
    {
        int n = snprintf(s, sizeof(s), "%s<", kern);
        for (const int *a = args.begin(); a != args.end(); a++)
            n += snprintf(s + n, sizeof(s) - n, a == args.begin() ? "%d" : ", %d", *a);
        snprintf(s + n, sizeof(s) - n, ">");
    }
};

// lds_optin_above of a kernel whose dynamic LDS never needs the opt-in
constexpr size_t NO_OPTIN = (size_t)-1;

template <typename T>
struct same_type {
    using type = T;
};

// The arguments convert to the kernel's own parameter types at the call, as
// in a <<<>>> launch, and stay on this frame until hipLaunchKernel has copied
// them: no allocation, no formatting.  The dynamic-LDS limit is raised when
// `lds` exceeds `lds_optin_above` bytes.
template <typename... P>
static int launch(Kernel<P...> k, dim3 grid, dim3 block, size_t lds, size_t lds_optin_above,
                  hipStream_t s, typename same_type<P>::type... args)
{
    const void *fn = (const void *)k.fn;
    if (!fn) {
        set_last_error_msg("launch: no kernel is built for these arguments");
        return NGMIX_ERR_BAD_ARG;
    }
    if (k.name) census(k.name);
    if (lds > lds_optin_above)
        NGMIX_HIP_CHECK(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize,
                                            (int)lds));
    void *argv[] = {(void *)&args...};
    (void)hipLaunchKernel(fn, grid, block, argv, lds, s);
    // (as after a <<<>>> launch: this also reports, and clears, an error that
    // an earlier asynchronous failure left behind)
    NGMIX_HIP_CHECK(hipGetLastError());
    return NGMIX_OK;
}

// (a kernel outside the census, named directly)
template <typename... P>
static int launch(void (*fn)(P...), dim3 grid, dim3 block, size_t lds, hipStream_t s,
                  typename same_type<P>::type... args)
{
    return launch(Kernel<P...>{fn, nullptr}, grid, block, lds, NO_OPTIN, s, args...);
}

// the kernel of the first row of a dispatch table that `match` accepts; no
// kernel when no row does (a table has no catch-all row)
template <typename Row, size_t N, typename Match>
static auto find_kernel(const Row (&rows)[N], Match match) -> decltype(rows[0].k)
{
    for (const Row &r : rows)
        if (match(r)) return r.k;
    return {nullptr, nullptr};
}

// f(std::integral_constant<int, V>) for the V of the list that equals v, the
// last of the list when none does
template <int V0, int... VS, typename F>
static auto for_int(int v, F &&f)
{
    if constexpr (sizeof...(VS) == 0)
        return f(std::integral_constant<int, V0>());
    else
        return v == V0 ? f(std::integral_constant<int, V0>())
                       : for_int<VS...>(v, std::forward<F>(f));
}

}  // namespace ngmix
