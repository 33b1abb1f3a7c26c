"""Row staging of the pair scan backward: every LDS-DMA source and destination offset, on the CPU.

The kernel's DMA (global_load_lds) checks no range, so the per-lane offset function
(scan_common.h: stage_src_elem / stage_dst_byte / stage_row_byte) is compiled into a stand-alone
host program with the address and undefined-behaviour sanitizers and run over every case the
kernel can meet: all L % 8 == 0 up to 136, nrows 0 .. 32, every chunk, both instructions, 64 lanes,
a dense and a channel-major row stride."""
import os
import shutil
import subprocess

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(REPO, "mamba-clip_amd", "csrc")

PROGRAM = r"""
#include <cstdint>
#include <cstdio>
#include <vector>
#include "scan_common.h"

using namespace mc::scan;

int main() {
  long checked = 0, bad = 0;
  const int wave_block = 4 * kStageArrayBytes;   // u, delta, dout, z of one wave
  for (int L = 8; L <= 136; L += 8) {
    const int nch = (L + kS - 1) / kS;
    const int64_t strides[3] = {L, 2 * (int64_t)L, 136 + 8};   // dense, channel-major at batch 2, padded rows
    for (int64_t ds : strides)
      for (int nrows = 0; nrows <= 32; ++nrows) {
        // the span the host validated: rows [0, max(nrows, 1)) of L elements each, as a byte map
        const int vrows = nrows > 0 ? nrows : 1;
        std::vector<unsigned char> valid((size_t)((vrows - 1) * ds + L), 0);
        for (int r = 0; r < vrows; ++r)
          for (int t = 0; t < L; ++t) valid[(size_t)(r * ds + t)] = 1;
        for (int c = 0; c < nch; ++c)
          for (int i = 0; i < 2; ++i)
            for (int lane = 0; lane < 64; ++lane) {
              const int64_t off = stage_src_elem(lane, i, c, nrows, L, ds);
              bool ok = off >= 0 && off + 8 <= (int64_t)valid.size() && off % 8 == 0;
              for (int e = 0; ok && e < 8; ++e) ok = valid[(size_t)(off + e)] != 0;
              // an unclamped piece is the row and the positions the sub-tile reads from that slot
              const int row = 16 * i + lane / 4, pos = c * kS + 8 * (lane % 4);
              if (row < nrows && pos + 8 <= L) ok = ok && off == row * ds + pos;
              const uint32_t dst = stage_dst_byte(lane, i);
              ok = ok && dst % 16 == 0 && dst + 16 <= (uint32_t)kStageArrayBytes;
              ok = ok && dst == stage_row_byte(row, 8 * (lane % 4));
              for (int arr = 0; arr < 4; ++arr) ok = ok && arr * kStageArrayBytes + dst + 16 <= (uint32_t)wave_block;
              ++checked;
              if (!ok) {
                if (++bad <= 10)
                  std::printf("BAD L=%d ds=%lld nrows=%d c=%d i=%d lane=%d off=%lld dst=%u\n", L, (long long)ds, nrows,
                              c, i, lane, (long long)off, dst);
              }
            }
      }
  }
  // the two instructions tile the array exactly once
  std::vector<int> hits(kStageArrayBytes / 16, 0);
  for (int i = 0; i < 2; ++i)
    for (int lane = 0; lane < 64; ++lane) ++hits[stage_dst_byte(lane, i) / 16];
  for (int h : hits) bad += h != 1;
  std::printf("checked %ld bad %ld\n", checked, bad);
  return bad ? 1 : 0;
}
"""


def _hipcc():
    for c in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if c and os.path.exists(c):
            return c
    return None


def test_stage_offsets_in_range(tmp_path):
    hipcc = _hipcc()
    assert hipcc, "hipcc not found: the staging offsets are checked by a compiled host program"
    src = tmp_path / "stage_offsets.hip"
    src.write_text(PROGRAM)
    exe = tmp_path / "stage_offsets"
    cmd = [hipcc, "--offload-arch=gfx950", "-O1", "-std=c++17", "-I", CSRC,
           "-Xarch_host", "-fsanitize=address,undefined", "-Xarch_host", "-fno-sanitize-recover=all",
           str(src), "-o", str(exe)]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout[-4000:], r.stderr[-4000:])
    assert "bad 0" in r.stdout, r.stdout
    # 17 lengths: sum of chunk counts x 3 strides x 33 row counts x 2 instructions x 64 lanes
    n_chunks = sum(-(-L // 32) for L in range(8, 137, 8))
    assert f"checked {n_chunks * 3 * 33 * 2 * 64} " in r.stdout, r.stdout
