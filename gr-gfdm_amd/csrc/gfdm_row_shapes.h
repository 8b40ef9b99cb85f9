// The shapes (K, M, L) whose row-lane kernels are compiled into the library: the ONE list.  The Makefile reads it (ROW_SHAPES) to
// build gfdm_rowlane_shape.hip once per shape and part, gfdm_rowlane.hip dispatches over it, and the sanitizer loop-back layer
// (tests/sanitize/loopback) reports the same shapes as compiled.  One entry per line, in the form the Makefile's sed expects.
#pragma once

#define GFDM_ROW_SHAPES(X) \
    X(64, 9, 2)            \
    X(32, 5, 2)            \
    X(32, 9, 2)            \
    X(128, 15, 4)          \
    X(256, 31, 2)          \
    X(64, 5, 2)            \
    X(64, 15, 2)           \
    X(128, 9, 2)           \
    X(128, 15, 2)          \
    X(128, 21, 2)          \
    X(4, 16, 2)            \
    X(4, 8, 2)             \
    X(96, 25, 2)
