"""bgzf_crc32_kernel on 512 MiB cut into ranges of 65 280 bytes (htslib's block size), per slicing width: libvtx_dev.so with
VTX_CRC_WIDTH = 16 / 8 / 4 / 16, one child process per width (the knob is read once), random bytes and ACGT text; device time from
vtx_last_crc_ms (event pair around the kernel), five launches each, GB/s from the fastest of the last four.  Every child checks a few
ranges against zlib.crc32.  GPU box:   python tools/crc32_bench.py"""
import json, os, subprocess, sys, zlib
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
if len(sys.argv) > 1 and sys.argv[1] == "child":
    import numpy as np
    from vartrix_amd import lib
    from vartrix_amd.abi import default_config
    kind = sys.argv[2]
    n = 512 << 20
    rng = np.random.default_rng(1)
    data = rng.integers(0, 256, n, dtype=np.uint8) if kind == "random" else np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, n)]
    step = 65280
    offsets = np.arange(0, n + 1, step, dtype=np.uint64)
    with lib.Context(default_config(n_barcodes=4), variant="dev") as ctx:
        ms = []
        for _ in range(5):
            got = ctx.debug_crc32(data, offsets)
            ms.append(ctx.crc_ms())
        for i in (0, 1, len(got) // 2, len(got) - 1):
            assert int(got[i]) == zlib.crc32(data[int(offsets[i]):int(offsets[i + 1])].tobytes()), i
    nb = int(offsets[-1])
    print(json.dumps(dict(width=int(os.environ["VTX_CRC_WIDTH"]), data=kind, bytes=nb, ranges=len(got), ms=[round(m, 4) for m in ms],
                          gb_per_s=round(nb / 1e6 / min(ms[1:]), 1))), flush=True)
    sys.exit(0)
for kind in ("random", "acgt"):
    for w in (16, 8, 4, 16):
        env = dict(os.environ, VTX_CRC_WIDTH=str(w), VTX_LIB_VARIANT="dev")
        r = subprocess.run(["timeout", "-k", "10", "150", sys.executable, os.path.abspath(__file__), "child", kind], env=env)
        if r.returncode != 0:
            print("child failed", w, r.returncode, flush=True)
            sys.exit(1)
