// pv_api_internal.h -- what the translation units of the C-ABI shim share (pv_api.cpp, pv_api_state.cpp): the handle structs, the
// thread-local error stack (defined in pv_api.cpp) and the exception guard.  Not installed; nothing here leaves the library.
//
// The stream-record entry points live in pv_api_state.cpp because they call Engine members that the host-only engine double of
// tests/abi_sanitizer does not define: pv_api.cpp alone must keep linking against that double.
#pragma once

#include <new>
#include <stdexcept>

#include "../../include/pv_koala.h"
#include "../../include/pv_koala_batch.h"
#include "kns_engine.h"

struct pv_koala {
    kns::Engine *engine;
};
struct pv_koala_batch {
    kns::Engine *engine;
};

namespace pv_api {

// the calling thread's error stack (at most 8 messages, drained by pv_get_error_stack): every entry point clears it first
void clear_errors();
void push_error(unsigned code, const char *fmt, ...);

// No C++ exception may cross the C ABI (the callers are ctypes / dlsym hosts: an escaping exception is std::terminate).  Every
// entry point that reaches engine code runs it through this: bad_alloc -> OUT_OF_MEMORY, anything else -> RUNTIME_ERROR.
template <class F>
pv_status_t guarded(F &&body) {
    try {
        return body();
    } catch (const std::bad_alloc &) {
        push_error(0x65, "Failed to allocate memory.");
        return PV_STATUS_OUT_OF_MEMORY;
    } catch (const std::length_error &) {
        push_error(0x65, "Failed to allocate memory.");
        return PV_STATUS_OUT_OF_MEMORY;
    } catch (const std::exception &e) {
        push_error(0x339, "Unexpected failure: %s", e.what());
        return PV_STATUS_RUNTIME_ERROR;
    } catch (...) {
        push_error(0x339, "Unexpected failure.");
        return PV_STATUS_RUNTIME_ERROR;
    }
}

}  // namespace pv_api
