#!/usr/bin/env python
"""Does ``hipMemsetAsync(p, 0, n)``, recorded by a stream capture as a memset node, zero its buffer on
every launch of the instantiated graph?  No project code is involved: the graph is
``[memset(buf, 0, n); buf += 1]``, the buffer is dirtied before every launch (alternating byte fills),
and after each launch the elements that are not exactly 1 are counted.

On the HIP runtime this was written against (7.0, MI355X) the first launch is right and every later
one leaves one dword in four of the buffer non-zero (index 2 mod 4, at the larger sizes index 0 mod 4
too; always at 4 KiB, in most runs at 4 MiB and 16 MiB); with the same fill before every launch all
launches are right.  That is why ``gnca_rollout_bwd_taps`` zeroes its accumulating rows with a
kernel.  One line per size; exit status 1 if any launch was wrong.

    python tools/memset_node_check.py
"""
from __future__ import annotations

import ctypes
import sys

import torch


def main() -> int:
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = ctypes.CDLL(path)          # (the runtime torch has loaded)
    hip.hipMemsetAsync.restype = ctypes.c_int
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
    wrong = False
    for nbytes in (4096, 4 << 20, 16 << 20):
        n = nbytes // 4
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=torch.cuda.Stream()):
            big = torch.empty(n + 1024, device=dev)          # from the graph's pool, as a workspace is
            buf = big[512:512 + n]
            rc = hip.hipMemsetAsync(buf.data_ptr(), 0, nbytes, torch.cuda.current_stream().cuda_stream)
            assert rc == 0, rc
            buf.add_(1.0)
        torch.cuda.synchronize()
        rows = []
        for i in range(4):
            big.view(torch.uint8).fill_(0xFF if i % 2 else 0x3F)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            bad = (buf != 1.0).nonzero().flatten()
            rows.append(f"launch {i + 1}: {bad.numel()} of {n} wrong" +
                        (f" (first at {bad[:4].tolist()}, value {buf[bad[0]].item()!r})" if bad.numel() else ""))
            wrong |= bad.numel() > 0
        print(f"memset node of {nbytes} B: " + "; ".join(rows), flush=True)
    return 1 if wrong else 0


if __name__ == "__main__":
    sys.exit(main())
