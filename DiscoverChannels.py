#!/usr/bin/env python3
"""Greedy EEG channel discovery on the MI355X: the discovery loop of the reference's
TestRetrieval_Perils_DiscoverChannels.py (:125-351), TestRetrieval_DiscoverChannels.py and
TestRetrieval_Perils_SaveChannelWiseOutputs.py, on the per-channel distance kernels.

    python DiscoverChannels.py --synthetic 2400 --dataset perils
    python DiscoverChannels.py --dataset spampinato --eeg_dataset ... --eeg_dataset_split ... --gallery_subject 1

Gallery and query are the first ``--samples_per_class`` items per class of the train and test parts of the [0.8, 0.2]
``random_split`` (seed 123, :62-63).  Every row carries its own label: the reference's lookup of the query label by
query position in the un-split dataset (:229-243) is not reproduced.  Plots, ICA, MNE and the per-image output dumps of
those scripts are not part of this tool.
"""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

DEFAULTS = {"perils": ("./data/eeg/theperils/spampinato-1-3RAW_with_mean_std.pth", ""),
            "spampinato": ("./data/eeg/spampinato/eeg_signals_raw_with_mean_std.pth",
                           "./data/eeg/spampinato/block_splits_by_image_all.pth")}


def build_parser():
    p = argparse.ArgumentParser('Greedy channel discovery by retrieval recall (MI355X).')
    p.add_argument('--dataset', type=str, default="perils", choices=["perils", "spampinato"])
    p.add_argument('--eeg_dataset', type=str, default="", help='default: the path the reference script of --dataset uses')
    p.add_argument('--eeg_dataset_split', type=str, default="")
    p.add_argument('--images_root', type=str, default="./data/images/imageNet_images")
    p.add_argument('--gallery_subject', type=int, default=1, choices=[0, 1, 2, 3, 4, 5, 6])
    p.add_argument('--time_low', type=int, default=20)
    p.add_argument('--time_high', type=int, default=480)
    p.add_argument('--topK', type=int, default=5)
    p.add_argument('--samples_per_class', type=int, default=30)
    p.add_argument('--fixed_channels', type=str, default="", help='comma-separated channels fixed from the start, in order')
    p.add_argument('--max_channels', type=int, default=0, help='stop once this many channels are accepted (0 = no limit)')
    p.add_argument('--budget_mb', type=int, default=4096, help='device memory for the per-channel distance matrices')
    p.add_argument('--synthetic', type=int, default=0, help='discover on N synthetic segments')
    p.add_argument('--synthetic_channels', type=int, default=0, help='default: 96 (perils) / 128 (spampinato)')
    p.add_argument('--synthetic_samples', type=int, default=500)
    p.add_argument('--seed', default=43, type=int)
    return p


def first_per_class(class_ids, indices, per_class):
    """The first ``per_class`` of ``indices`` of every class, classes ascending (label_wise_data[i]["eeg"][:30], :151-175)."""
    by_class = {}
    for i in indices:
        by_class.setdefault(int(class_ids[i]), []).append(int(i))
    return [i for c in sorted(by_class) for i in by_class[c][:per_class]]


def main(argv=None):
    from cerebralsignalnetworks_amd.channel_discovery import discover_channels
    from cerebralsignalnetworks_amd.dataset import EEGDataset
    from cerebralsignalnetworks_amd.trainer import split_indices

    FLAGS = build_parser().parse_args(argv)
    print(FLAGS)
    torch.cuda.set_device(0)
    device = torch.device("cuda", 0)
    if FLAGS.synthetic:
        channels = FLAGS.synthetic_channels or (96 if FLAGS.dataset == "perils" else 128)
        dataset = EEGDataset(synthetic=FLAGS.synthetic, synthetic_channels=channels, synthetic_samples=FLAGS.synthetic_samples,
                             time_low=0, time_high=FLAGS.synthetic_samples, seed=FLAGS.seed, device=device,
                             flavour=FLAGS.dataset)
    else:
        path, split = DEFAULTS[FLAGS.dataset]
        split = FLAGS.eeg_dataset_split or split
        spamp = FLAGS.dataset == "spampinato"
        dataset = EEGDataset(eeg_signals_path=FLAGS.eeg_dataset or path, imagesRoot=FLAGS.images_root,
                             eeg_splits_path=split if spamp and os.path.exists(split) else None,
                             subject=FLAGS.gallery_subject if spamp else 1, flavour=FLAGS.dataset, time_low=0,
                             time_high=FLAGS.time_high, device=device)
    train_idx, test_idx = split_indices(len(dataset), (0.8, 0.2), seed=123)          # :62-63
    class_ids = dataset.labels.tolist()
    gallery_rows = first_per_class(class_ids, train_idx.tolist(), FLAGS.samples_per_class)
    query_rows = first_per_class(class_ids, test_idx.tolist(), FLAGS.samples_per_class)
    eeg = dataset.eeg_all                                                             # [N, C, T], resident
    gallery = eeg[torch.as_tensor(gallery_rows, device=eeg.device)]
    query = eeg[torch.as_tensor(query_rows, device=eeg.device)]
    gallery_labels = [dataset.getLabelbyIndex(i) for i in gallery_rows]
    query_labels = [dataset.getLabelbyIndex(i) for i in query_rows]
    time_high = min(FLAGS.time_high, eeg.shape[2])
    start = [int(c) for c in FLAGS.fixed_channels.split(",") if c.strip()]
    print(f"gallery {tuple(gallery.shape)} query {tuple(query.shape)} window [{FLAGS.time_low}, {time_high}) topK {FLAGS.topK}")

    result = discover_channels(gallery, query, gallery_labels, query_labels, dataset, topK=FLAGS.topK,
                               time_low=FLAGS.time_low, time_high=time_high, start=start,
                               max_channels=FLAGS.max_channels or None, budget_bytes=FLAGS.budget_mb << 20)
    fixed = list(start)
    for metrics, best in zip(result.rounds, result.best):
        for ch, (recall, precision) in metrics.items():
            print(f"TS {fixed}[{ch}] Overall Recall :{recall} Overall Precision: {precision}")
        if best:
            subset, (recall, precision) = best
            print(f"best score channel: {''.join(f',{c}' for c in subset)}  with Scores: "
                  f"{{'Recall': {recall}, 'Precision': {precision}}}")
        fixed = result.order[:len(fixed) + 1]
    if result.stopped.startswith("found no channel"):
        print(f"found no channel better than last iteration. final channels: {result.order}")
    else:
        print(f"stopped: {result.stopped}. final channels: {result.order}")
    return result


if __name__ == "__main__":
    main()
