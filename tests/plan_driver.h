// What the host drivers of the stages' plan headers share (the ten tests/*_plan_driver.cpp with a Call struct: epipolar,
// guided, refit, homography, pose, chain, resect, resect_refine, tracks, bundle): the tally of checks with the first failure
// kept, and REJECT: a valid Call, one change to it, and the expectation that it is refused.
#pragma once
#include <cstdio>

struct Tally {
    long checked = 0, bad = 0;
    char first[200] = "-";
    void expect(bool ok, const char* what, unsigned long long a = 0, unsigned long long b = 0, unsigned long long c = 0) {
        ++checked;
        if (!ok && !bad++) std::snprintf(first, sizeof first, "%s:%llu,%llu,%llu", what, a, b, c);
    }
};

// `args`: the Tally in scope; `Call`: the driver's valid call with bool valid().
#define REJECT(what, stmt)            \
    {                                 \
        Call c;                       \
        stmt;                         \
        args.expect(!c.valid(), what); \
    }
