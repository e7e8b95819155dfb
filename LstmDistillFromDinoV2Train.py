#!/usr/bin/env python3
"""MI355X trainer with the command-line / checkpoint surface of the reference's
LstmDistillFromDinoV2Train.py (flags :150-225, loop :351-424, checkpoint :411-419).

    python LstmDistillFromDinoV2Train.py --synthetic 256 --batch_size 16 --num_epochs 1
    torchrun --nproc-per-node 8 LstmDistillFromDinoV2Train.py --synthetic 65536 --batch_size 256 ...

Differences that the hardware forces, all opt-in or documented in DESIGN.md: data and frozen
teacher embeddings are resident on the GPU; one process per GPU with RCCL gradient all-reduce
(the reference initialises gloo and never shards, :234,286); ``--hyperprams`` is parsed with
``ast.literal_eval`` (the reference ``eval``s it, :247); DINOv2 embeddings come from
``--teacher_features`` (.npy) or are synthetic -- ``torch.hub`` (:144-146) needs a network.
"""
import argparse
import ast
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


class Flavour:
    """What differs between the reference's two trainers of this loop.  `perils` = LstmDistillFromDinoV2Train.py
    (RMSprop 1e-3 :329, Model(128, 96, 2, include_top=True) + FeatureDistributionLoss :323-365, ONE checkpoint name
    :414,419); `spampinato` = LstmDistillFromDinoV2TrainSpampinato.py (AdamW 1e-4 :378, Model(128, 128, layers=4,
    include_top=False) :368, loss_fn_kd with alpha / temperature from --hyperprams :107-121,288-296, weights-only resume
    from --custom_model_weights when the file exists :369-371, first best checkpoint lstm_dinov2_epoch_{E}_best_loss.pth
    then lstm_dinov2_epochs_{EPOCHS}_best_loss.pth :467-475, utils/EEGDataset.py with subject + split file :310-317)."""

    def __init__(self, name, learning_rate, num_epochs, eeg_dataset, eeg_dataset_split, hyperprams, optimizer, loss,
                 hidden_size, lstm_layers, dataset_flavour):
        self.name, self.learning_rate, self.num_epochs = name, learning_rate, num_epochs
        self.eeg_dataset, self.eeg_dataset_split, self.hyperprams = eeg_dataset, eeg_dataset_split, hyperprams
        self.optimizer, self.loss, self.hidden_size, self.lstm_layers = optimizer, loss, hidden_size, lstm_layers
        self.dataset_flavour = dataset_flavour

    def checkpoint_path(self, log_dir, epoch, epochs, first_best):
        if self.name == "spampinato":
            return (f"{log_dir}/lstm_dinov2_epoch_{epoch}_best_loss.pth" if first_best
                    else f"{log_dir}/lstm_dinov2_epochs_{epochs}_best_loss.pth")
        return f"{log_dir}/lstm_dinov2_best_loss.pth"


PERILS = Flavour("perils", 0.001, 100, "./data/eeg/theperils/spampinato-1-IMAGE_BLOCK_RAW_with_mean_std.pth",
                 "./data/eeg/block_splits_by_image_all.pth",
                 "{'ce_loss_weight': 0.50, 'soft_target_loss_weight':0.50,'alpha': 1,'temperature':2}",
                 "rmsprop", "featdist", 96, 2, "perils")
SPAMPINATO = Flavour("spampinato", 0.0001, 200, "./data/eeg/spampinato/eeg_signals_raw_with_mean_std.pth",
                     "./data/eeg/spampinato/block_splits_by_image_all.pth",
                     "{'ce_loss_weight': 0.50, 'soft_target_loss_weight':0.50,'alpha': 0,'temperature':2}",
                     "adamw", "kd", 128, 4, "spampinato")


def build_parser(flavour=PERILS):
    p = argparse.ArgumentParser('LSTM distillation from DINOv2 embeddings (MI355X).')
    p.add_argument('--learning_rate', type=float, default=flavour.learning_rate)
    p.add_argument('--num_epochs', type=int, default=flavour.num_epochs)
    p.add_argument('--batch_size', type=int, default=16, help='per-process batch size')
    p.add_argument('--log_dir', type=str, default='./logs/DinoV2LstmDistillv2sdsad/')
    p.add_argument('--gallery_subject', type=int, default=1, choices=[0, 1, 2, 3, 4, 5, 6])
    p.add_argument('--query_subject', type=int, default=1, choices=[0, 1, 2, 3, 4, 5, 6])
    p.add_argument('--eeg_dataset', type=str, default=flavour.eeg_dataset)
    p.add_argument('--images_root', type=str, default="./data/images/imageNet_images")
    p.add_argument('--eeg_dataset_split', type=str, default=flavour.eeg_dataset_split)
    p.add_argument('--mode', type=str, default="train")
    p.add_argument('--custom_model_weights', type=str, default="")
    p.add_argument('--search_gallery', type=str, default="train")
    p.add_argument('--query_gallery', type=str, default="test")
    p.add_argument('--topK', type=int, default=5)
    p.add_argument('--gallery_tranformation_type', type=str, default="eeg2eeg", choices=["img", "img2eeg", "eeg", "eeg2eeg"])
    p.add_argument('--query_tranformation_type', type=str, default="eeg2eeg", choices=["img", "img2eeg", "eeg", "eeg2eeg"])
    p.add_argument('--hyperprams', type=str, default=flavour.hyperprams)
    p.add_argument('--seed', default=43, type=int)
    p.add_argument('--num_workers', default=4, type=int)
    p.add_argument("--dist_url", default="env://", type=str)
    p.add_argument("--local_rank", default=0, type=int)
    # --- additions (SURVEY.md section 5 "Config / flags") ---
    p.add_argument('--synthetic', type=int, default=0, help='train on N synthetic 128x500 segments')
    p.add_argument('--synthetic_samples', type=int, default=440 if flavour.name == "spampinato" else 500,
                   help='samples per synthetic segment (BASELINE.json: 128 x 500; Spampinato split 128 x 440)')
    p.add_argument('--teacher_features', type=str, default="", help='.npy [N,D] precomputed frozen-teacher embeddings')
    p.add_argument('--hidden_size', type=int, default=flavour.hidden_size, help='lstm_size (reference call sites: 96 / 128)')
    p.add_argument('--lstm_layers', type=int, default=flavour.lstm_layers)
    p.add_argument('--lstm_dropout', type=float, default=0.0,
                   help='nn.LSTM(dropout=p): dropout between the LSTM layers while training (0 = off; validation and '
                        'retrieval run in eval mode, without it)')
    p.add_argument('--bidirectional', action='store_true',
                   help='nn.LSTM(bidirectional=True): the encoder runs in both directions (BiLSTM) and fc takes the final '
                        'state of each, 2 * hidden_size features; with --lstm_dropout the concatenated output of every '
                        'layer but the top one is dropped once, as torch drops it')
    p.add_argument('--resident_lstm', action='store_true',
                   help='hidden_size <= 128: the LSTM runs the steps of a chunk inside one launch per layer, W_hh in '
                        'registers (CSN_LSTM_RESIDENT plans), with the bits of the per-step cell kernels')
    p.add_argument('--readout', type=str, default="last", choices=["last", "mean", "max", "attn"],
                   help='what fc reads of the LSTM output sequence: its last step, or its mean / maximum over time, reduced '
                        'inside the library (no parameter depends on these), or "attn": their weighted mean under a learned query '
                        '(the checkpoint then holds lstm.attn_query); evaluate a checkpoint with the readout it was trained with')
    p.add_argument('--output_size', type=int, default=384)
    p.add_argument('--loss', type=str, default=flavour.loss, choices=["featdist", "cosine", "kd", "barlow", "contrastive", "contrastive_bank"],
                   help='contrastive_bank: InfoNCE against the bank of every image\'s teacher row (all images are negatives at every '
                        'step; a mean over rows, so --accum_steps and ragged shards work)')
    p.add_argument('--contrastive_temperature', type=float, default=0.07,
                   help='--loss contrastive / contrastive_bank: the fixed temperature of the InfoNCE loss (logit scale = 1 / temperature)')
    p.add_argument('--contrastive_mask', type=str, default="image", choices=["image", "class", "none"],
                   help='--loss contrastive: rows that are not each other\'s negatives -- the same image (shown to several '
                        'subjects), the same class, or none; --loss contrastive_bank: class = the other images of the '
                        'positive\'s class are not negatives, image / none = every other image is (a bank row is one image)')
    p.add_argument('--optimizer', type=str, default=flavour.optimizer, choices=["rmsprop", "adamw", "adam", "lars"])
    p.add_argument('--dtype', type=str, default="bf16", choices=["bf16", "f32"])
    p.add_argument('--fs', type=float, default=1000.0, help='sampling rate for the band-pass design')
    p.add_argument('--filter_order', type=int, default=3, choices=[0, 3, 4, 5], help='0 = no band-pass')
    p.add_argument('--time_low', type=int, default=20)
    p.add_argument('--time_high', type=int, default=480)
    p.add_argument('--validation_frequency', type=int, default=5)
    p.add_argument('--accum_steps', type=int, default=1,
                   help='micro-batches per optimiser step: each batch runs as this many equal parts whose gradients are '
                        'summed on the device (batch_size must be a multiple; a shorter last batch of an epoch is cut '
                        'to one)')
    p.add_argument('--fused_optimizer', action='store_true',
                   help='adamw / adam / lars as fused HIP steps over the flat parameter buffer (rmsprop always is)')
    p.add_argument('--clip_grad_norm', type=float, default=0.0,
                   help='clip the global gradient norm to this value once per optimiser step (the coefficient of '
                        'torch.nn.utils.clip_grad_norm_, decided on the device); 0 = off')
    p.add_argument('--skip_nonfinite', action='store_true',
                   help='do not take an optimiser step whose gradient holds a NaN or an Inf (parameters and optimiser state '
                        'stay as they were); the epoch line counts such steps; needs a flat optimiser (rmsprop, or '
                        '--fused_optimizer)')
    p.add_argument('--fused_loss', action='store_true',
                   help='featdist / kd / barlow / contrastive / contrastive_bank: loss value and gradient from fused HIP calls in float64 '
                        '(csn_distill_loss, csn_barlow_corr + csn_barlow_grad, csn_contrastive_lse + csn_contrastive_grad, '
                        'csn_bank_contrastive) '
                        'instead of a chain of torch ops; does nothing with --loss cosine (always fused)')
    p.add_argument('--compat_label_bug', action='store_true',
                   help='reproduce the batch-local label lookup of transformEEGDataLSTMByList')
    p.add_argument('--normalize_embeddings', action='store_true',
                   help='retrieval leg: L2-normalise gallery and query embeddings first, so that the L2 ranking is the '
                        'cosine ranking (what --loss contrastive trains)')
    p.add_argument('--device_eval', action='store_true',
                   help='retrieval leg: the embeddings stay on the device, class hits are counted there (csn_topk_merge, '
                        'csn_topk_class_metrics) and the host folds per-class integers into the same Recall / Precision / '
                        'top1 (not with --compat_label_bug, which keeps the host form)')
    return p


def normalize_rows(rows):
    """--normalize_embeddings: rows / max(|row|, 1e-12) of a [N,D] tensor or of a list of numpy rows."""
    if torch.is_tensor(rows):
        return torch.nn.functional.normalize(rows, dim=1, eps=1e-12)
    return [r / max(float(np.linalg.norm(r)), 1e-12) for r in rows]


class _KdParams:
    alpha = 0.5
    temperature = 2.0


class _LoaderEmbedder:
    """What the reference hands to ``dataset.transformEEGDataLSTMByList`` is its model; items of a loader over the dataset
    are ``eeg[T, C]`` as ``__getitem__`` returns them, so here the callable also applies the step's preprocessing (the
    fused band-pass + z-score takes the stored channel-first layout)."""

    def __init__(self, trainer):
        self.trainer = trainer

    def __call__(self, eeg_btc):
        return self.trainer.model(self.trainer.embed(eeg_btc.transpose(1, 2).contiguous()))


def init_distributed():
    """One process per GPU; RCCL when launched by torchrun, single process otherwise
    (utils/utils.py:467-503 exits without a GPU -- so does this)."""
    if not torch.cuda.is_available():
        print('Does not support training without GPU.')
        sys.exit(1)
    if "RANK" in os.environ and "WORLD_SIZE" in os.environ and int(os.environ["WORLD_SIZE"]) > 1:
        local = int(os.environ.get("LOCAL_RANK", 0))
        if os.environ.get("CSN_SINGLE_DEVICE"):      # rehearsal of the multi-rank path on a one-GPU box (as in bench.py)
            local = 0
        torch.cuda.set_device(local)
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        backend = os.environ.get("CSN_DIST_BACKEND", "nccl")     # "nccl" is RCCL on ROCm; gloo only for rehearsals
        if backend == "nccl":
            dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local))
        else:
            dist.init_process_group(backend=backend)
        return dist.get_rank(), dist.get_world_size(), local
    torch.cuda.set_device(0)
    return 0, 1, 0


def main(argv=None, flavour=PERILS):
    from cerebralsignalnetworks_amd import Model, EEGFilters
    from cerebralsignalnetworks_amd.dataset import EEGDataset
    from cerebralsignalnetworks_amd.retrieval import evaluate_device, evaluate_distributed, evaluate_full
    from torch.utils.data import DataLoader, Subset
    from cerebralsignalnetworks_amd.trainer import DistillTrainer, shard_indices, split_indices
    from cerebralsignalnetworks_amd.losses import HyperParams

    FLAGS, _unparsed = build_parser(flavour).parse_known_args(argv)
    if FLAGS.accum_steps < 1 or FLAGS.batch_size % FLAGS.accum_steps != 0:
        raise SystemExit(f"--accum_steps {FLAGS.accum_steps}: must be >= 1 and divide --batch_size {FLAGS.batch_size}")
    if not FLAGS.clip_grad_norm >= 0:
        raise SystemExit(f"--clip_grad_norm {FLAGS.clip_grad_norm}: must be >= 0 (0 = off)")
    rank, world, local = init_distributed()
    is_main = rank == 0
    if is_main:
        print(FLAGS)
    os.makedirs(FLAGS.log_dir, exist_ok=True)
    hyper = ast.literal_eval(FLAGS.hyperprams)
    kd = _KdParams()
    kd.alpha = hyper.get("alpha", kd.alpha)                 # (Parameters.alpha / .temperature of the Spampinato script, :288-296)
    kd.temperature = hyper.get("temperature", kd.temperature)
    torch.manual_seed(FLAGS.seed)
    device = torch.device("cuda", local)

    if FLAGS.synthetic:
        dataset = EEGDataset(synthetic=FLAGS.synthetic, synthetic_samples=FLAGS.synthetic_samples, time_low=0,
                             time_high=FLAGS.synthetic_samples, seed=FLAGS.seed, device=device,
                             feature_dim=FLAGS.output_size, compat_label_bug=FLAGS.compat_label_bug)
    else:
        spamp = flavour.dataset_flavour == "spampinato"       # utils/EEGDataset.py: subject + split file (:310-317)
        dataset = EEGDataset(eeg_signals_path=FLAGS.eeg_dataset, imagesRoot=FLAGS.images_root,
                             eeg_splits_path=FLAGS.eeg_dataset_split if spamp and os.path.exists(FLAGS.eeg_dataset_split) else None,
                             subject=FLAGS.gallery_subject if spamp else 1, flavour=flavour.dataset_flavour,
                             time_low=FLAGS.time_low, time_high=FLAGS.time_high, device=device,
                             compat_label_bug=FLAGS.compat_label_bug)
        if not FLAGS.teacher_features:
            raise SystemExit("--teacher_features is required with a real dataset (torch.hub DINOv2 needs a network)")
        dataset.set_features(np.load(FLAGS.teacher_features, allow_pickle=False))
    N = len(dataset)
    features_length = dataset.features_all.shape[1]
    C = dataset.eeg_all.shape[1]

    train_idx, val_idx = (ix.to(device) for ix in split_indices(N, (0.8, 0.2), seed=43))      # random_split, :289-290

    dtype = torch.bfloat16 if FLAGS.dtype == "bf16" else torch.float32
    include_top = FLAGS.loss == "featdist"
    model = Model(input_size=C, lstm_size=FLAGS.hidden_size, lstm_layers=FLAGS.lstm_layers,
                  output_size=features_length, include_top=include_top, compute_dtype=dtype,
                  dropout=FLAGS.lstm_dropout, bidirectional=FLAGS.bidirectional, resident=FLAGS.resident_lstm,
                  readout=FLAGS.readout).to(device)
    if flavour.name == "spampinato":
        if os.path.exists(FLAGS.custom_model_weights):           # :369-371: resume only if the file is there, strict keys
            model.load_state_dict(torch.load(FLAGS.custom_model_weights, map_location="cpu", weights_only=True))
            if is_main:
                print(f"loaded  {FLAGS.custom_model_weights}")
    elif FLAGS.custom_model_weights:
        sd = torch.load(FLAGS.custom_model_weights, map_location="cpu", weights_only=True)
        model.load_state_dict(sd, strict=False)
    sos = EEGFilters(FLAGS.fs, order=FLAGS.filter_order).sos if FLAGS.filter_order else None
    trainer = DistillTrainer(model, sos, loss=FLAGS.loss, lr=FLAGS.learning_rate, optimizer=FLAGS.optimizer,
                             nepochs=max(FLAGS.num_epochs, HyperParams.warmup_teacher_temp_epochs + 1), kd_params=kd,
                             accum_steps=FLAGS.accum_steps, fused_optimizer=FLAGS.fused_optimizer,
                             fused_loss=FLAGS.fused_loss, contrastive_temperature=FLAGS.contrastive_temperature,
                             max_grad_norm=FLAGS.clip_grad_norm or None, skip_nonfinite=FLAGS.skip_nonfinite)

    pos_all = None
    if FLAGS.loss == "contrastive_bank":        # the bank of the WHOLE dataset's images, once: the teacher is frozen
        bank, pos_all, bank_class = dataset.image_bank()
        trainer.set_bank(bank, bank_class if FLAGS.contrastive_mask == "class" else None)
        if is_main:
            print(f"contrastive_bank: {bank.shape[0]} images in the bank, mask {FLAGS.contrastive_mask}")

    def batches(idx, epoch, shuffle, multiple_of=1):
        shard = idx[shard_indices(len(idx), epoch, FLAGS.seed, rank, world, shuffle=shuffle).to(device)]
        for s in range(0, len(shard), FLAGS.batch_size):
            b = shard[s:s + FLAGS.batch_size]
            b = b[:len(b) - len(b) % multiple_of]       # (a shorter last batch: whole micro-batches only)
            if len(b):
                yield b

    def loss_kw(b):
        """--loss contrastive: the group ids of the batch, by --contrastive_mask; contrastive_bank: the rows' positives."""
        if FLAGS.loss == "contrastive_bank":
            return {"positives": pos_all[b]}
        if FLAGS.loss != "contrastive" or FLAGS.contrastive_mask == "none":
            return {}
        return {"groups": (dataset.image_ids_dev if FLAGS.contrastive_mask == "image" else dataset.labels_dev)[b]}

    def labels_of(ix):
        return [dataset.getLabelbyIndex(int(i)) for i in ix.cpu()]

    best_val_loss, best_val_loss_epoch, history = None, -1, []
    for EPOCH in range(FLAGS.num_epochs):
        losses = []
        for b in batches(train_idx, EPOCH, True, FLAGS.accum_steps):
            losses.append(trainer.train_step(dataset.eeg_all[b], dataset.features_all[b], dataset.labels_dev[b], EPOCH,
                                             **loss_kw(b)))
        trainer.check_device_status()      # per epoch: a timed-out in-kernel hand-off must not pass silently
        epoch_loss = float(torch.stack(losses).mean().item())                    # one sync per epoch, not per step
        skipped = f" skipped {trainer.skipped_steps()}" if FLAGS.skip_nonfinite else ""       # (steps not taken so far)
        if EPOCH % FLAGS.validation_frequency == 0 and EPOCH > 0:
            model.eval()
            if FLAGS.compat_label_bug:
                # the reference's own retrieval leg, call for call (:383-389): both loaders go through
                # dataset.transformEEGDataLSTMByList, whose labels are looked up by the position INSIDE the batch
                # (PerilsEEGDataset.py:336-338) -- Recall / Precision come out as the reference prints them, not as
                # retrieval quality.  Every rank walks the whole loaders, like the reference's ranks.
                embedder = _LoaderEmbedder(trainer)
                loaders = [DataLoader(Subset(dataset, ix.tolist()), batch_size=FLAGS.batch_size, shuffle=False)
                           for ix in (train_idx, val_idx)]
                gallery_features, gallery_labels = dataset.transformEEGDataLSTMByList(model=embedder, data_loader=loaders[0])
                query_features, query_labels = dataset.transformEEGDataLSTMByList(model=embedder, data_loader=loaders[1])
                if FLAGS.normalize_embeddings:
                    gallery_features, query_features = normalize_rows(gallery_features), normalize_rows(query_features)
                r = evaluate_full(FLAGS, gallery_features, query_features, gallery_labels, query_labels, dataset)
            else:
                # each rank embeds ITS shard of the gallery and of the queries; the neighbour lists are gathered
                g_ix = train_idx[shard_indices(len(train_idx), 0, FLAGS.seed, rank, world, shuffle=False).to(device)]
                q_ix = val_idx[shard_indices(len(val_idx), 0, FLAGS.seed, rank, world, shuffle=False).to(device)]
                if world > 1:       # (the sampler pads a shard by wrapping around: drop the duplicates again)
                    g_ix = g_ix[: len(range(rank, len(train_idx), world))]
                    q_ix = q_ix[: len(range(rank, len(val_idx), world))]
                gallery = trainer.embed_all(dataset.eeg_all[g_ix], FLAGS.batch_size)
                query = trainer.embed_all(dataset.eeg_all[q_ix], FLAGS.batch_size)
                if FLAGS.normalize_embeddings:
                    gallery, query = normalize_rows(gallery), normalize_rows(query)
                if FLAGS.device_eval and world == 1:
                    r = evaluate_device(FLAGS, gallery, query, labels_of(g_ix), labels_of(q_ix), dataset)
                else:
                    r = evaluate_distributed(FLAGS, list(gallery.cpu().numpy()), list(query.cpu().numpy()), labels_of(g_ix),
                                             labels_of(q_ix), dataset, on_device=FLAGS.device_eval)
            # validation loss over ALL ranks' shards: sum of the batch losses and their count, one all-reduce, so that
            # the best-checkpoint decision below is the same on every rank and covers the whole validation split
            vsum = torch.zeros(2, device=device, dtype=torch.float64)
            with torch.no_grad():
                for b in batches(val_idx, 0, False):
                    out = model(trainer.embed(dataset.eeg_all[b]))
                    vsum[0] += trainer.compute_loss(out, dataset.features_all[b], dataset.labels_dev[b], EPOCH,
                                                       **loss_kw(b)).double()
                    vsum[1] += 1
            if world > 1:
                if dist.get_backend() == "nccl":
                    dist.all_reduce(vsum)
                else:                       # gloo rehearsal: host tensors
                    host = vsum.cpu()
                    dist.all_reduce(host)
                    vsum = host
            val_epoch_loss = float((vsum[0] / vsum[1]).item())
            improved = best_val_loss is None or val_epoch_loss < best_val_loss
            if improved:
                first = best_val_loss is None
                best_val_loss, best_val_loss_epoch = val_epoch_loss, EPOCH
                if is_main:
                    torch.save(model.state_dict(), flavour.checkpoint_path(FLAGS.log_dir, EPOCH, FLAGS.num_epochs, first))
            if is_main:
                print(f"Overall Recall :{r['Recall_Total']} Overall Precision: {r['Precision_Total']} top1: {r['top1']:.4f}")
                print(f"EPOCH {EPOCH} train_loss: {round(epoch_loss, 6)} val_loss: {round(val_epoch_loss, 6)} "
                      f"T: {HyperParams.T} best val loss: {best_val_loss} on epoch: {best_val_loss_epoch}{skipped}")
        elif is_main:
            print(f"EPOCH {EPOCH} train_loss: {round(epoch_loss, 6)} T: {HyperParams.T}{skipped}")
        history.append(epoch_loss)
    if is_main and best_val_loss is None and flavour.name == "perils":
        torch.save(model.state_dict(), f"{FLAGS.log_dir}/lstm_dinov2_best_loss.pth")
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()
    return history


if __name__ == "__main__":
    main()
