"""Score a sample batch against a reference batch: Inception Score, FID, sFID, precision and recall -- the five lines of the
reference's ``evaluations/evaluator.py REF.npz SAMPLE.npz`` (main() :29-84), computed on the MI355X
(autodiffusion_amd/evaluator.py).

    python scripts/evaluator.py REF.npz SAMPLE.npz --inception_path pt_inception.pth [--batch_size 64] [--mode tf1]
                                [--save_ref_stats ref_stats.npz]

Both files hold uint8 NHWC images as ``arr_0`` (what scripts/classifier_sample.py writes); a reference batch may instead
carry its statistics (``mu, sigma, mu_s, sigma_s``), which are then used as they are -- its ``arr_0`` still gives the
precision / recall features.  The lines also go to ``<SAMPLE>_eval.log`` next to the sample file.
``--save_ref_stats OUT.npz`` writes the reference's ``mu, sigma, mu_s, sigma_s``: ``scripts/search_ea.py --ref_path OUT.npz``
reads it as it is (the reference pickles a FIDStatistics instead, evaluator.py:47-55).
``--kid True [--kid_subsets 100 --kid_subset_size 1000 --kid_seed 0]`` appends a sixth line, ``KID: <mean> +- <std>``: the unbiased
cubic-kernel MMD^2 over subset draws (project-defined, autodiffusion_amd/kid.py); ``--save_ref_feats OUT.npz`` writes the
reference's pool3 features as ``feats`` for ``scripts/search_ea.py --fitness kid --ref_feats OUT.npz``.

The Inception-v3 checkpoint (pt_inception-2015-12-05 state_dict with ``fc.weight``) is not in this image.  Without
``--inception_path`` the CLI exits; ``--inception_random True`` opts in to random weights (a random softmax head included)
for throughput runs and tests, and every line is then tagged.
"""
import argparse
import logging
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

RANDOM_TAG = " [RANDOM Inception weights: not a quality metric]"


def create_argparser():
    from autodiffusion_amd.script_util import str2bool
    p = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    p.add_argument("ref_batch", help="path to the reference batch .npz")
    p.add_argument("sample_batch", help="path to the sample batch .npz")
    p.add_argument("--inception_path", default="", help="Inception-v3 state_dict (.pth / .safetensors) with fc.weight")
    p.add_argument("--inception_random", type=str2bool, default=False, help="allow random Inception weights (tests only)")
    p.add_argument("--batch_size", type=int, default=64)
    p.add_argument("--mode", default="tf1", choices=["tf1", "pt"], help="input handling of the extractor (inception.features)")
    p.add_argument("--save_ref_stats", default="", help="write the reference's mu, sigma, mu_s, sigma_s to this .npz")
    p.add_argument("--kid", type=str2bool, default=False, help="append a sixth line, 'KID: <mean> +- <std>' (autodiffusion_amd/kid.py)")
    p.add_argument("--kid_subsets", type=int, default=100, help="number of subset draws of the KID line")
    p.add_argument("--kid_subset_size", type=int, default=1000, help="rows drawn from each set per subset (no larger than either set)")
    p.add_argument("--kid_seed", type=int, default=0, help="np.random.RandomState seed of the subset draws")
    p.add_argument("--save_ref_feats", default="", help="write the reference's pool3 features as `feats` (fp32 [m, 2048]) to this .npz")
    return p


def log_path(sample_batch: str) -> str:
    return os.path.splitext(sample_batch)[0] + "_eval.log"


def load_inception(args, device):
    import torch
    from autodiffusion_amd.evaluator import random_inception
    from autodiffusion_amd.inception import InceptionV3
    if args.inception_path:
        if args.inception_path.endswith(".safetensors"):
            from safetensors.torch import load_file
            sd = load_file(args.inception_path)
        else:
            sd = torch.load(args.inception_path, map_location="cpu", weights_only=True)
        net = InceptionV3().to(device)
        net.load_state_dict(sd)
        if net.fc_weight is None:
            raise SystemExit("evaluator.py: the checkpoint has no fc.weight [classes, 2048]: the Inception Score needs it")
        return net
    return random_inception(device)


def main(argv=None):
    args = create_argparser().parse_args(argv)
    if not args.inception_path and not args.inception_random:
        raise SystemExit("evaluator.py: give --inception_path (the pt_inception-2015-12-05 state_dict with fc.weight): scores on "
                         "random weights are meaningless (--inception_random True opts in for throughput runs and tests)")
    import numpy as np
    import torch
    from autodiffusion_amd.evaluator import Evaluator

    tag = RANDOM_TAG if not args.inception_path else ""
    device = torch.device("cuda", torch.cuda.current_device())
    evaluator = Evaluator(load_inception(args, device), batch_size=args.batch_size, mode=args.mode)

    log = logging.getLogger("adm_evaluator")
    log.setLevel(logging.INFO)
    log.propagate = False
    log.handlers.clear()
    fmt = logging.Formatter("%(asctime)s %(message)s", datefmt="%m/%d %I:%M:%S %p")
    for h in (logging.StreamHandler(sys.stdout), logging.FileHandler(log_path(args.sample_batch))):
        h.setFormatter(fmt)
        log.addHandler(h)

    print("computing reference batch activations...")
    ref_acts = evaluator.read_activations(args.ref_batch)
    print("computing/reading reference batch statistics...")
    ref_stats, ref_stats_spatial = evaluator.read_statistics(args.ref_batch, ref_acts)
    if args.save_ref_stats:
        np.savez(args.save_ref_stats, mu=ref_stats.mu, sigma=ref_stats.sigma, mu_s=ref_stats_spatial.mu,
                 sigma_s=ref_stats_spatial.sigma)
    if args.save_ref_feats:
        np.savez(args.save_ref_feats, feats=np.asarray(ref_acts[0], dtype=np.float32))
    print("computing sample batch activations...")
    sample_acts = evaluator.read_activations(args.sample_batch)
    print("computing/reading sample batch statistics...")
    sample_stats, sample_stats_spatial = evaluator.read_statistics(args.sample_batch, sample_acts)

    log.info(str(args.sample_batch))
    log.info("Computing evaluations...")
    log.info("Inception Score: " + str(evaluator.compute_inception_score(sample_acts[0])) + tag)
    log.info("FID: " + str(sample_stats.frechet_distance(ref_stats)) + tag)
    log.info("sFID: " + str(sample_stats_spatial.frechet_distance(ref_stats_spatial)) + tag)
    prec, recall = evaluator.compute_prec_recall(ref_acts[0], sample_acts[0])
    log.info("Precision:" + str(prec) + tag)
    log.info("Recall:" + str(recall) + tag)
    if args.kid:
        kid_mean, kid_std = evaluator.compute_kid(ref_acts[0], sample_acts[0], args.kid_subsets, args.kid_subset_size, args.kid_seed)
        log.info("KID: " + str(kid_mean) + " +- " + str(kid_std) + tag)
    for h in log.handlers:
        h.close()


if __name__ == "__main__":
    main()
