// What a kernel driver or a state object returns to the ABI layer: 0 or one of
// these (errno-like values; status_of() in xcg_api_host.h maps each to its ABI
// status).  Part of xcg_args.h, kept apart because it needs no HIP:
// xcg_volume.cpp and the CPU harnesses include it alone.
#pragma once

constexpr int XCG_RC_NOENT = -2;       // no such file / volume
constexpr int XCG_RC_HIP = -5;         // a HIP runtime call failed
constexpr int XCG_RC_NOMEM = -12;
constexpr int XCG_RC_INVAL = -22;
constexpr int XCG_RC_OVERFLOW = -75;   // an internal table overflowed
constexpr int XCG_RC_NOTSUP = -95;
