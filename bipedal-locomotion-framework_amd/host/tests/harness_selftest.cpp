/**
 * @file harness_selftest.cpp
 * test_harness.h under test (tests/test_host_harness.py reads the output): one host case and one
 * device-flagged case, both passing and neither touching a device.
 * usage: blf_harness_selftest [cpu|gpu|all] [N]   (N: the host case fails N checks more)
 */
#include <cstdlib>

#include "test_harness.h"

static int g_toFail = 0;

static void hostCase()
{
    REQUIRE(true);
    for (int i = 0; i < g_toFail; ++i) REQUIRE(i < 0);
}

static void deviceFlaggedCase()
{
    REQUIRE_FALSE(false);
}

int main(int argc, char** argv)
{
    if (argc > 2) g_toFail = std::atoi(argv[2]);
    return runCases(argc, argv, {
        {"harness host case", false, hostCase},
        {"harness device-flagged case", true, deviceFlaggedCase},
    });
}
