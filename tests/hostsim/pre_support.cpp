// TEST INFRASTRUCTURE: what csrc/preprocess.hip needs from the rest of the library when it is built alone for the host simulator
// (tests/_hostsim_preprocess.py): the error plumbing and the negative version number that marks a simulator build (both live in block.hip in the product).
#include <cstdarg>
#include <cstdio>
static thread_local char g_err[512] = "";
void maed_set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
extern "C" const char* maed_last_error(void) { return g_err; }
extern "C" int maed_version(void) { return -100; }
