#!/usr/bin/env python3
"""Static counts per kernel symbol of a gfx950 assembly listing (hipcc -S --cuda-device-only).

For every kernel: MFMAs, packed fp32 VALU instructions (v_pk_fma_f32 / v_pk_mul_f32 / v_pk_add_f32) between the first and the
last v_mfma of the symbol, single v_fma / v_fmac / v_mul / v_add f32 in the same region, VGPRs and scratch instructions.

usage: count_pk.py listing.s [substring of the demangled name ...]
"""
import re
import subprocess
import sys


def kernels(path):
    name, body = None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m:
            name, body = m.group(1), []
            continue
        if name is None:
            continue
        body.append(line)
        if line.lstrip().startswith(".end_amdhsa_kernel"):
            yield name, body
            name = None


def count(body):
    ins = [l.split("//")[0].split(";")[0].strip() for l in body]
    ins = [l for l in ins if l and not l.startswith(".") and not l.endswith(":")]
    mf = [i for i, l in enumerate(ins) if l.startswith("v_mfma")]
    region = ins[mf[0]:mf[-1] + 1] if mf else []

    def n(prefix, where):
        return sum(1 for l in where if l.startswith(prefix))
    vgpr = next((int(m.group(1)) for l in body for m in [re.search(r"\.amdhsa_next_free_vgpr\s+(\d+)", l)] if m), -1)
    agpr = next((int(m.group(1)) for l in body for m in [re.search(r"\.amdhsa_accum_offset\s+(\d+)", l)] if m), -1)
    return dict(mfma=len(mf), pk_fma=n("v_pk_fma_f32", region), pk_mul=n("v_pk_mul_f32", region), pk_add=n("v_pk_add_f32", region),
                # v_fma_mix_f32: the IEEE-half library's affine, an fp32 fma that converts its 16-bit operand itself
                fma=n("v_fma_f32", region) + n("v_fmac_f32", region) + n("v_fma_mix_f32", region), mul=n("v_mul_f32", region), add=n("v_add_f32", region),
                vgpr=vgpr, accum_offset=agpr, scratch=n("scratch_", ins))


def main():
    path, want = sys.argv[1], sys.argv[2:]
    rows = []
    for name, body in kernels(path):
        dem = subprocess.run(["c++filt", name], capture_output=True, text=True).stdout.strip()
        dem = re.sub(r"^void ", "", dem).replace("(anonymous namespace)::", "").split("(")[0]
        if want and not any(w in dem for w in want):
            continue
        rows.append((dem, count(body)))
    print("symbol | mfma | pk_fma pk_mul pk_add (in the MFMA region) | fma mul add (single, same region) | vgprs (arch+acc) | scratch instructions")
    for dem, c in sorted(rows):
        print(f"{dem} | {c['mfma']} | {c['pk_fma']} {c['pk_mul']} {c['pk_add']} | {c['fma']} {c['mul']} {c['add']} | {c['vgpr']} | {c['scratch']}")


if __name__ == "__main__":
    main()
