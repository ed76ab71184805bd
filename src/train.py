"""ref src/train.py surface without Lightning or Hydra: compose the configs, instantiate the data module and the module, drive
`OneProtLitModule.fit_steps` over the train loader for `trainer.max_steps` steps, run the validation hooks, write a weights checkpoint.

    python src/train.py [data=oneprot] [model=oneprot_text] [key=value ...]

`group=option` picks a config group's file (configs/<group>/<option>.yaml), every other key=value is a YAML value on a dotted key, e.g.
data.modalities.text.dataset.data_dir=/data/pretrain trainer.max_steps=100 ckpt_path=/ckpts/last.ckpt.  configs/train.yaml composes the model, trainer and
paths groups; the data group (default: configs/data/oneprot.yaml, the reference's composition) is composed here beside it."""
import logging
import os
import sys

_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if _ROOT not in sys.path:
    sys.path.insert(0, _ROOT)

import torch  # noqa: E402
import yaml  # noqa: E402

from oneprot_amd import data as _data  # noqa: E402
from oneprot_amd.config import compose, instantiate  # noqa: E402

log = logging.getLogger("train")
CONFIG_DIR = os.path.join(_ROOT, "configs")


def compose_config(overrides=(), config_dir=CONFIG_DIR):
    """the training config: configs/train.yaml with the data group beside it; overrides: "key=value" strings"""
    given = {}
    for ov in overrides:
        key, _, value = ov.partition("=")
        given[key] = yaml.safe_load(value)
    data_option = given.pop("data", "oneprot")
    data_keys = {k: v for k, v in given.items() if k.startswith("data.")}
    cfg = compose(config_dir, "train", overrides={k: v for k, v in given.items() if k not in data_keys})
    if "data" not in cfg:
        cfg["data"] = compose(config_dir, f"data/{data_option}", overrides=data_keys)["data"]
    return cfg


def to_device(batch, device):
    """a collate function's tuple with its two inputs on `device` (tensors, PackedTokens, PackedMsa and GraphBatch all have .to)"""
    sequence_input, modality_input, modality, raw = batch
    return sequence_input.to(device), modality_input.to(device), modality, raw


def train_batches(loader, device, max_steps):
    """{modality: batch} dicts of the min_size loader, over as many epochs as max_steps needs"""
    step = 0
    while step < max_steps:
        empty = True
        for batch in loader:
            empty = False
            yield {m: to_device(b, device) for m, b in batch.items()}
            step += 1
            if step >= max_steps:
                return
        if empty:
            raise RuntimeError("the train loader is empty: no modality has a train dataset with rows")


def train(cfg, device=None):
    """(module, data module) after trainer.max_steps training steps and one pass over the validation loader"""
    device = torch.device(device if device is not None else "cuda")
    if cfg.get("seed"):
        torch.manual_seed(cfg["seed"])
    log.info(f"Instantiating datamodule <{cfg['data']['_target_']}>")
    datamodule = instantiate(cfg["data"])
    datamodule.setup("fit")
    log.info(f"Instantiating model <{cfg['model']['_target_']}>")
    module = instantiate(cfg["model"]).to(device)
    if cfg.get("ckpt_path"):
        log.info("Loading model weights from checkpoint!")
        _data.load_weights_only(module, cfg["ckpt_path"])
    max_steps = int(cfg["trainer"].get("max_steps", -1))
    if max_steps < 1:
        raise ValueError("trainer.max_steps must be a positive number of steps: this driver counts steps, not epochs")
    loss = module.fit_steps(train_batches(datamodule.train_dataloader(), device, max_steps))
    log.info(f"train/loss after {max_steps} steps: {float(loss.detach()) if loss is not None else None}")
    val = datamodule.val_dataloader()
    if len(val):
        module.eval()
        for batch, batch_idx, dataloader_idx in val:
            module.validation_step(to_device(batch, device), batch_idx, dataloader_idx)
        module.on_validation_epoch_end()
    out_dir = cfg.get("paths", {}).get("output_dir", ".")
    os.makedirs(out_dir, exist_ok=True)
    path = os.path.join(out_dir, "last.ckpt")
    _data.save_checkpoint(module, path)
    log.info(f"wrote {path}")
    return module, datamodule


def main(argv=None):
    logging.basicConfig(level=logging.INFO, format="%(asctime)s - %(levelname)s - %(message)s")
    return train(compose_config(sys.argv[1:] if argv is None else argv))


if __name__ == "__main__":
    main()
