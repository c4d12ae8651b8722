/**
 * @file test_harness.h
 * What every test program under host/tests/ shares: the check counters, REQUIRE / REQUIRE_FALSE, and
 * runCases, which runs a table of cases and reports them.
 *   usage of a program: <binary> [cpu|gpu|all]   (default all; cpu runs the cases that need no device)
 *   stdout: one "name ... ok" / "name ... FAILED" line per case that ran, then "N checks, M failed"
 *   stderr: "  FAILED file:line: condition" per failed check
 *   exit status: 0 if no check failed, 1 if one did, 2 for a mode that is none of the three
 * tests/host_binaries.py is the reader of these lines.
 */
#pragma once

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

static int g_failed = 0, g_checks = 0;
#define REQUIRE(cond)                                                                          \
    do {                                                                                       \
        ++g_checks;                                                                            \
        if (!(cond)) {                                                                         \
            ++g_failed;                                                                        \
            std::fprintf(stderr, "  FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);           \
        }                                                                                      \
    } while (0)
#define REQUIRE_FALSE(cond) REQUIRE(!(cond))

struct Case
{
    const char* name;
    bool device;   // needs a GPU: run in the modes gpu and all
    std::function<void()> fn;
};

inline int runCases(int argc, char** argv, const std::vector<Case>& cases)
{
    const std::string which = argc > 1 ? argv[1] : "all";
    if (which != "cpu" && which != "gpu" && which != "all")
    {
        std::fprintf(stderr, "%s: unknown mode '%s' (cpu, gpu or all)\n", argv[0], which.c_str());
        return 2;
    }
    const bool cpu = which != "gpu", gpu = which != "cpu";
    int width = 0;
    for (const Case& c : cases) width = std::max(width, static_cast<int>(std::strlen(c.name)));
    for (const Case& c : cases)
    {
        if (c.device ? !gpu : !cpu) continue;
        const int before = g_failed;
        c.fn();
        std::printf("%-*s %s\n", width, c.name, g_failed == before ? "ok" : "FAILED");
    }
    std::printf("%d checks, %d failed\n", g_checks, g_failed);
    return g_failed != 0;
}
