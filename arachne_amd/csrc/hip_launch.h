// hip_launch.h -- the one place the library's host code starts a HIP kernel, and the one check of a HIP call's result.  gfx950 only.
#pragma once
#include <hip/hip_runtime.h>
#include <stdexcept>
#include <string>

namespace arx {

// what a failed HIP call or launch throws: "<the call as written, or the launch's name>: <HIP's error string>".  A type of its own so that
// a caller may tell it from its other errors (the index build puts its "index build: " in front: hip_index_build.h)
struct HipError : std::runtime_error { using std::runtime_error::runtime_error; };
inline void hip_check(hipError_t e, const char *what) { if (e != hipSuccess) throw HipError(std::string(what) + ": " + hipGetErrorString(e)); }
#define ARX_HIP_CHECK(x) ::arx::hip_check((x), #x)

// What a launch is called in that text: the kernel, the class or variant of it where one call site starts several (-1: none), and the
// caller's name for the work (a Scope name: it tells the functor of a generic kernel such as k_items<F>), as "kernel[cls] (scope)"
struct LaunchName {
	const char *kernel, *scope = nullptr; int cls = -1;
	LaunchName(const char *kernel_, const char *scope_ = nullptr, int cls_ = -1) : kernel(kernel_), scope(scope_), cls(cls_) {}
	std::string str() const { return kernel + (cls < 0 ? std::string() : "[" + std::to_string(cls) + "]") + (scope ? " (" + std::string(scope) + ")" : std::string()); }
};
template <class T> struct as_declared { using type = T; };

// Starts `kernel` and checks the launch at once, so that a launch the runtime refuses (grid, LDS size, arguments) is reported under its own
// name and not under that of a later one.  The arguments are taken as the kernel's own parameter types, so what converts implicitly at a
// raw launch converts here and nothing else does (a literal 0 or nullptr is a null pointer, void * is not a T *).
template <class... P> inline void hip_launch(const LaunchName &name, void (*kernel)(P...), dim3 grid, dim3 block, size_t lds_bytes, hipStream_t stream, typename as_declared<P>::type... args)
{
	hipLaunchKernelGGL(kernel, grid, block, lds_bytes, stream, args...);
	const hipError_t e = hipGetLastError();
	if (e != hipSuccess) hip_check(e, name.str().c_str());
}

} // namespace arx
