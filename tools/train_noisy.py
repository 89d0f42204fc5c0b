"""Train a denoiser on a directory of images that are ALREADY noisy and have no clean counterpart: Neighbor2Neighbor pairs in front
of the ordinary training step (blind_image_denoising_amd/neighbor.py), validated by Stein's unbiased risk estimate
on some of the same kind of images.  It reads only the files it is given and adds no noise.

    python tools/train_noisy.py pipeline.json noisy_photos/ run/ --gamma 2 --validate held_out/ --every 500

CONFIG is a pipeline configuration (model, loss, train, dataset sections); its dataset `inputs` are replaced by IMAGES, its noise
options are dropped, and `train.self_supervised` is set from the arguments (a section already in the file supplies the defaults).
--validate names directories of noisy images for the risk records (default: IMAGES itself; the first 16 files); after the run the records of
OUTPUT/risk.jsonl are printed as tables."""
import argparse
import copy
import json
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(__file__), ".."))
import blind_image_denoising_amd as bf                     # noqa: E402


def pipeline(config, images, gamma=None, ramp=None, validate=None, every=None, sigma=None, method=None, probes=None):
    """the configuration the tool trains with: `config` with IMAGES as its dataset and the self_supervised section filled in"""
    cfg = copy.deepcopy(config)
    dataset = dict(cfg.get("dataset", {}))
    for k in ("additional_noise", "multiplicative_noise"):
        dataset.pop(k, None)
    dataset["inputs"] = [{"directory": str(images)}]
    cfg["dataset"] = dataset
    section = dict(cfg["train"].get("self_supervised") or {"type": "neighbor2neighbor"})
    validation = dict(section.get("validation") or {})
    for key, value in (("gamma", gamma), ("ramp", ramp)):
        if value is not None:
            section[key] = value
    validation["inputs"] = [str(v) for v in validate] if validate else validation.get("inputs") or [str(images)]
    for key, value in (("every", every), ("sigma", sigma), ("method", method), ("probes", probes)):
        if value is not None:
            validation[key] = value
    section["validation"] = validation
    cfg["train"]["self_supervised"] = section
    bf.parse_self_supervised_config(cfg["train"])          # refuse a bad section before anything is built
    return cfg


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("config")
    ap.add_argument("images", help="a directory of noisy images")
    ap.add_argument("output", help="the model directory: checkpoints, epoch_N/, final/, risk.jsonl")
    ap.add_argument("--gamma", type=float, default=None, help="weight of the regulariser (the paper uses 1..2 for synthetic, up to 8 for real noise)")
    ap.add_argument("--no-ramp", dest="ramp", action="store_false", default=None, help="the full gamma from the first step")
    ap.add_argument("--validate", nargs="+", default=None, help="directories of noisy images for the risk records")
    ap.add_argument("--every", type=int, default=None, help="optimizer steps between risk records (default 0: one per epoch)")
    ap.add_argument("--sigma", type=float, default=None, help="noise standard deviation in grey levels (default: estimated)")
    ap.add_argument("--method", choices=bf.risk.METHODS, default=None)
    ap.add_argument("--probes", type=int, default=None)
    ap.add_argument("--max-steps", type=int, default=None)
    args = ap.parse_args(argv)
    if not os.path.isdir(args.images):
        ap.error(f"{args.images} is not a directory")
    cfg = pipeline(bf.load_config(args.config), args.images, args.gamma, args.ramp, args.validate, args.every, args.sigma, args.method,
                   args.probes)
    model, history = bf.train_loop(cfg, args.output, max_steps=args.max_steps)
    print(f"{len(history)} steps, loss {history[0]:.4f} -> {history[-1]:.4f}; model in {os.path.join(args.output, 'final')}")
    with open(os.path.join(args.output, "risk.jsonl")) as f:
        for line in f:
            record = json.loads(line)
            for r in record["risk"]["batches"] + [record["risk"]["aggregate"]]:      # strict JSON wrote null for inf / NaN
                r.update({k: float("nan") for k, v in r.items() if v is None})
            print(f"step {record['step']} (epoch {record['epoch']})")
            print(bf.format_risk_report(record["risk"]))
    return model, history


if __name__ == "__main__":
    main()
