"""CPU: the decision behind return code -3 of the check libraries (csrc/check_runner.h, guards_intact): a device output comes
back between two guard records of 0xAA bytes, and one changed byte in either record is a lane that stored outside its own
record.  The header's HIP-free part is compiled with g++ into a stand-alone program.  Needs no GPU."""
import os
import subprocess

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "python-bls_amd", "csrc")

# one line per case: payload bytes, the changed byte's offset in guard | payload | guard (-1: none), guards_intact
DRIVER = r'''
#include "check_runner.h"
#include <stdio.h>
#include <vector>
static void row(size_t payload, long at) {
    std::vector<unsigned char> back(payload + 2 * check::GUARD, 0xAA);
    for (size_t j = 0; j < payload; j++) back[check::GUARD + j] = (unsigned char)(j * 7 + 1);
    if (at >= 0) back[at] ^= 0x01;
    printf("%zu %ld %d\n", payload, at, check::guards_intact(back.data(), payload) ? 1 : 0);
}
int main() {
    const size_t sizes[3] = {0, 4, 1028};
    for (size_t payload : sizes) {
        const long G = (long)check::GUARD, P = (long)payload;
        row(payload, -1);
        for (long j = 0; j < P; j++) row(payload, G + j);
        row(payload, 0); row(payload, G - 1); row(payload, G + P); row(payload, 2 * G + P - 1);
    }
    return 0;
}
'''


def test_one_written_guard_byte_is_seen_and_payload_bytes_are_not(tmp_path):
    src, exe = tmp_path / "driver.cpp", tmp_path / "driver"
    src.write_text(DRIVER)
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wall", "-Werror", "-I", CSRC, "-o", str(exe), str(src)])
    rows = [tuple(int(x) for x in line.split()) for line in subprocess.run([str(exe)], capture_output=True, text=True, check=True).stdout.split("\n") if line]
    G = 256
    for payload in (0, 4, 1028):
        got = {at: ok for p, at, ok in rows if p == payload}
        edges = (0, G - 1, G + payload, 2 * G + payload - 1)
        assert set(got) == {-1} | set(range(G, G + payload)) | set(edges), payload
        assert got[-1] == 1, "a clean buffer"
        assert all(got[at] == 1 for at in range(G, G + payload)), "a changed payload byte is no written guard"
        assert [got[at] for at in edges] == [0, 0, 0, 0], "first and last byte of the front guard, first and last of the back guard"
    assert len(rows) == 3 * 5 + 4 + 1028
