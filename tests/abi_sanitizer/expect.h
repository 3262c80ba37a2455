// What the drivers of the C ABI (tests/abi_*/driver.cpp) share: the expectation counter, the error stack's drain and two small helpers.
// TEST INFRASTRUCTURE: never linked into the product.
#pragma once

#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "pv_koala.h"
#include "pv_koala_batch.h"

static int g_fail = 0;
#define EXPECT(cond)                                              \
    do {                                                          \
        if (!(cond)) {                                            \
            fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #cond); \
            ++g_fail;                                             \
        }                                                         \
    } while (0)

// drains the thread's stack; returns its depth and the first message
static int drain(std::string *first = nullptr) {
    char **stack = nullptr;
    int32_t depth = -1;
    const pv_status_t st = pv_get_error_stack(&stack, &depth);
    if (depth > 0) {
        EXPECT(st == PV_STATUS_SUCCESS && stack != nullptr);
        for (int i = 0; i < depth; ++i) EXPECT(stack[i] != nullptr && strlen(stack[i]) > 17);  // "<7 hex> <8 hex>: text"
        if (first) *first = stack[0];
        pv_free_error_stack(stack);
    } else {
        EXPECT(st == PV_STATUS_INVALID_STATE && depth == 0 && stack == nullptr);  // nothing pending: nothing to free
    }
    return depth;
}

static inline bool has(const std::string &s, const char *what) { return s.find(what) != std::string::npos; }

static inline pv_koala_batch_config_t config(int32_t B, int32_t frames, int32_t samples, int32_t rate, pv_koala_sample_format_t fmt) {
    pv_koala_batch_config_t c;
    memset(&c, 0, sizeof(c));
    c.struct_size = (int32_t) sizeof(c);
    c.num_streams = B, c.max_frames_per_call = frames, c.max_samples_per_call = samples;
    c.precision = PV_KOALA_PRECISION_FP32, c.sample_rate = rate, c.sample_format = fmt;
    return c;
}
