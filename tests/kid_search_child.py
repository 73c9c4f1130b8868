"""Child process of tests/test_hip_kid.py: scripts/search_ea.py's main() with two observers -- every KID fitness with the rows it
was computed from, and every pooled_rows call with what went in, what came out and over which backend -- written to an .npz.

    python tests/kid_search_child.py OUT.npz <flags of scripts/search_ea.py>

A process of its own because the command line initialises a process group (one per process)."""
import importlib.util
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    out, argv = sys.argv[1], sys.argv[2:]
    import torch.distributed as dist
    from autodiffusion_amd import kid, search
    from autodiffusion_amd.dist_util import collectives_on
    fits, pools = [], []
    fit0, pool0 = search.EvolutionSearcher._kid_fitness, kid.pooled_rows

    def fit(self, acc, local):
        v = fit0(self, acc, local)
        fits.append((self.last_rows.detach().cpu().numpy().copy(), float(v)))
        return v

    def pool(rows, group=None, local=False):
        res = pool0(rows, group, local)
        through = bool(collectives_on(group)) and not local
        pools.append((rows.detach().cpu().numpy().copy(), res.detach().cpu().numpy().copy(), through,
                      dist.get_backend() if dist.is_initialized() else "", str(res.device)))
        return res

    search.EvolutionSearcher._kid_fitness = fit
    kid.pooled_rows = pool          # _kid_fitness looks the name up at call time
    spec = importlib.util.spec_from_file_location("search_ea_cli", os.path.join(ROOT, "scripts", "search_ea.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    cli.main(argv)
    data = {"count": np.array(len(fits))}
    for i, (rows, v) in enumerate(fits):
        data[f"rows{i}"], data[f"value{i}"] = rows, np.array(v)
    for i, (a, b, through, backend, device) in enumerate(pools):
        data[f"pool_in{i}"], data[f"pool_out{i}"] = a, b
        data[f"pool_how{i}"] = np.array([str(through), backend, device])
    np.savez(out, **data)


if __name__ == "__main__":
    main()
