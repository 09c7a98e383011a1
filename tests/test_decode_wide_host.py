"""Host side of the wide decode call (up to 64 samples as four groups of 16) and of MusicLM.forward(fine_windows_together=True):
limits, scratch sizes against the header's macros, and the order in which fine windows are stacked along the batch axis.  No GPU."""
import os
import subprocess

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _models():
    from open_musiclm_amd import open_musiclm as M
    big = M.create_coarse_transformer(dim=1024, depth=1, heads=8, num_coarse_quantizers=3, precision="bf16")
    small = M.create_coarse_transformer(dim=128, depth=1, heads=2, num_coarse_quantizers=3, precision="bf16")
    return big, small


def test_wide_call_limits():
    """max_call_batch is 64 exactly where max_batch is 16 (the matrix-core step kernels); wide=True moves supports() to that limit and
    changes nothing for a call that exists today."""
    from open_musiclm_amd import decode
    big, small = _models()
    for precision in ("bf16", "fp16", "fp16ff"):
        assert decode.max_call_batch(big, precision) == 64
        assert decode.max_batch(big, precision) == 16
    assert decode.max_call_batch(big, "bf16x3") == 8
    assert decode.max_call_batch(small, "bf16") == 8
    assert not decode.supports(big, 17, "bf16")
    assert decode.supports(big, 17, "bf16", wide=True) and decode.supports(big, 64, "bf16", wide=True)
    assert not decode.supports(big, 65, "bf16", wide=True)
    assert not decode.supports(small, 9, "bf16", wide=True)
    assert decode.supports(big, 16, "bf16", wide=True) and decode.supports(small, 8, "bf16", wide=True)
    assert not decode.supports(big, 9, wide=True)                # no precision named: the conservative limit, as without the keyword
    # a wide batch takes the lo planes of "fp16ff" wherever a 16-sample batch does
    ff = _models()[0]
    assert decode.lo_planes_ok(ff, 64) == decode.lo_planes_ok(ff, 16) and decode.lo_planes_ok(ff, 17) == decode.lo_planes_ok(ff, 16)


@pytest.mark.parametrize("D,Fp", [(1024, 2752), (1024, 3072), (1024, 64)])
def test_scratch_sizes_equal_the_header_macros(tmp_path, D, Fp):
    """What CachedDecoder allocates for B in {16, 17, 64} (decode.scratch_sizes) equals OMLM_DECODE_*_B of include/omlm.h, and for
    B <= 16 the per-group macros the header has always had."""
    from open_musiclm_amd import decode
    batches = [1, 8, 16, 17, 24, 40, 64]
    src = tmp_path / "sizes.c"
    lines = ['#include <stdio.h>', f'#include "{os.path.join(ROOT, "include", "omlm.h")}"', 'int main(void) {']
    for B in batches:
        lines.append(f'  printf("%d %d %d\\n", (int)OMLM_DECODE_LN_PARTS_B({B}, {D}, {Fp}), (int)OMLM_DECODE_SPLITK_FLOATS_B({B}, {D}), '
                     f'(int)OMLM_DECODE_SPLITK_CNT_B({B}, {D}));')
    lines.append(f'  printf("%d %d %d\\n", (int)(3 * OMLM_DECODE_LN_PARTS({D}, {Fp})), (int)OMLM_DECODE_SPLITK_FLOATS({D}), (int)OMLM_DECODE_MAX_BATCH);')
    lines.append('  return 0; }')
    src.write_text("\n".join(lines))
    exe = tmp_path / "sizes"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    rows = [[int(v) for v in ln.split()] for ln in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.splitlines()]
    for B, row in zip(batches, rows):
        s = decode.scratch_sizes(B, D, Fp)
        assert [s["ln_parts"], s["splitk_ws"], s["splitk_cnt"]] == row, (B, s, row)
    per_group = rows[-1]
    assert per_group[2] == decode.DEC4_GMAX * decode.DEC4_NB == 64
    for B in (1, 8, 16):                                        # one group: today's sizes
        s = decode.scratch_sizes(B, D, Fp)
        assert s["ln_parts"] == per_group[0] and s["splitk_ws"] == per_group[1] and s["splitk_cnt"] == max((D + 15) // 16, 16)
    s = decode.scratch_sizes(64, D, Fp)                         # four groups: four times, and a ticket per (group, tile) and per sample
    assert s["ln_parts"] == 4 * per_group[0] and s["splitk_ws"] == 4 * per_group[1] and s["splitk_cnt"] == max(4 * ((D + 15) // 16), 64)
    assert decode.scratch_sizes(17, D, Fp)["splitk_ws"] == 2 * per_group[1]


def test_decode_args_mirror_still_matches_the_header(tmp_path):
    """The wide call adds no field: the mirror's size is the header struct's (the field-by-field test lives in test_host_logic)."""
    import ctypes
    from open_musiclm_amd import decode
    src = tmp_path / "sz.c"
    src.write_text(f'#include <stdio.h>\n#include "{os.path.join(ROOT, "include", "omlm.h")}"\n'
                   'int main(void) { printf("%zu\\n", sizeof(omlm_decode_args)); return 0; }\n')
    exe = tmp_path / "sz"
    subprocess.run(["gcc", "-std=c99", "-o", str(exe), str(src)], check=True)
    assert int(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout) == ctypes.sizeof(decode.DecodeArgs)


def test_window_helpers_round_trip_in_window_major_order():
    """_stack_windows puts window w of sample b at row w * B + b; _unstack_windows returns the originals."""
    from open_musiclm_amd import open_musiclm as M
    B, T, Q, size = 3, 10, 2, 2
    t = torch.arange(B * T * Q).reshape(B, T, Q)
    wins = M._windows(t, size, size)
    W = len(wins)
    assert W == 5
    stacked = M._stack_windows(wins)
    assert stacked.shape == (W * B, size, Q)
    for w in range(W):
        for b in range(B):
            assert torch.equal(stacked[w * B + b], t[b, w * size:(w + 1) * size])
    back = M._unstack_windows(stacked, W)
    assert len(back) == W and all(torch.equal(x, y) for x, y in zip(back, wins))
    assert torch.equal(torch.cat(back, dim=1), t)               # cut back into windows and joined along time: the sequence again
    with pytest.raises(AssertionError):
        M._unstack_windows(stacked[:-1], W)


def test_the_flag_is_documented_as_a_permission():
    from open_musiclm_amd import open_musiclm as M
    doc = M.MusicLM.__doc__
    assert "fine_windows_together" in doc and "permission" in doc and "random stream" in doc
