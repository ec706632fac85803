"""Re-ranker bases (mirror of the reference's models/BaseRerankerModel.py:15-132): a re-ranker scores the impression lists of a
frozen base ranker.  `RerankModel` / `RerankSeqModel` load `<ranker_name>Impression` from ./model/<ranker_name>Impression/ (a yaml of
its flags and its checkpoint, as the reference does; `history_max` is not taken from the yaml), freeze it, and their Dataset's
collate_batch runs it on the device and adds to the feed dict

    scores        the ranker's prediction with padded slots at -inf          padding_mask   true on padded slots
    position      each slot's rank under those scores (the double sort)      u_v, i_v       the ranker's user / candidate vectors
    his_v         (RerankSeqModel) the ranker's item vectors of the clicked history

The mask is built from the TRAINING list widths in every phase, as the reference does (:75-78), and the re-rankers index a position
table of that width: evaluation widths that differ from the training widths are refused at construction.
Not carried over: --tuneranker 1 (refused: the ranker's forward runs under no_grad inside collate_batch, there is nothing to tune).
One deliberate difference: the reference's head re-draws every Linear / Embedding below `self` after the ranker was loaded
(`self.apply(self.init_weights)` reaches self.ranker), which leaves a ranker of noise; `restore_ranker` loads the checkpoint again
after the head's init, so the same random stream initialises the head and the ranker is the trained one.
"""
import copy
import importlib
from typing import List

import numpy as np
import torch
import yaml

from models.BaseImpressionModel import ImpressionModel, ImpressionSeqModel
from utils import utils

RANKER_PACKAGES = ('models.general', 'models.sequential')


def find_ranker_class(ranker_name):
    """<ranker_name>Impression of models/general/<ranker_name>.py or models/sequential/<ranker_name>.py (reference :54)"""
    for pkg in RANKER_PACKAGES:
        try:
            mod = importlib.import_module('{}.{}'.format(pkg, ranker_name))
        except ModuleNotFoundError:
            continue
        cls = getattr(mod, ranker_name + 'Impression', None)
        if cls is not None:
            return cls
    raise ValueError('--ranker_name {0!r}: no class {0}Impression in {1}'.format(ranker_name, RANKER_PACKAGES))


def rank_positions(scores, all_mask):
    """(masked scores, position): padded slots at -inf, position = the rank of each slot under the masked scores (reference :79-81).
    Among the padded slots (all -inf) the order is the sort's; they take the ranks the valid slots leave free."""
    scores = torch.where(all_mask, scores, torch.full_like(scores, -np.inf))
    _, order = scores.sort(dim=1, descending=True)
    _, position = order.sort(dim=1)
    return scores, position


class RerankModel(ImpressionModel):
    reader = 'ImpressionReader'
    runner = 'ImpressionRunner'
    extra_log_args = ['tuneranker']

    @staticmethod
    def parse_model_args(parser):
        parser.add_argument('--ranker_name', type=str, default='BPRMF', help='Base ranker')
        parser.add_argument('--ranker_config_file', type=str, default='BPRMF.yaml', help='Base ranker config file')
        parser.add_argument('--ranker_model_file', type=str, default='BPRMF.pt', help='Base ranker model file')
        parser.add_argument('--tuneranker', type=int, default=0, help='if 1, continue to train ranker (not supported)')
        return ImpressionModel.parse_model_args(parser)

    def __init__(self, args, corpus):
        super().__init__(args, corpus)
        self.ranker_name = args.ranker_name
        self.ranker_config = args.ranker_config_file
        self.ranker_model = args.ranker_model_file
        self.tuneranker = args.tuneranker
        if self.tuneranker:
            raise ValueError('--tuneranker 1 is not supported: the base ranker runs frozen, under no_grad, inside collate_batch')
        if (self.test_max_pos_item, self.test_max_neg_item) != (self.train_max_pos_item, self.train_max_neg_item):
            raise ValueError('re-rankers need --test_max_pos_item / --test_max_neg_item equal to the training widths ({} / {}): the '
                             'padding mask and the position table are built from the training widths in every phase, got {} / {}'
                             .format(self.train_max_pos_item, self.train_max_neg_item, self.test_max_pos_item, self.test_max_neg_item))
        self.load_ranker(args, corpus)

    def ranker_paths(self):
        folder = './model/{}Impression/'.format(self.ranker_name)
        return folder + self.ranker_config, folder + self.ranker_model

    def load_ranker(self, args, corpus):
        config_path, self._ranker_model_path = self.ranker_paths()
        with open(config_path, 'r', encoding='utf-8') as f:
            config = yaml.load(f.read(), Loader=yaml.FullLoader) or {}
        ranker_args = copy.deepcopy(args)
        for k, v in config.items():
            if k != 'history_max':
                setattr(ranker_args, k, v)
        cls = find_ranker_class(self.ranker_name)
        self.ranker = cls(ranker_args, corpus)
        self.ranker.device = ranker_args.device
        self.ranker.return_vectors = True      # SASRecImpression hands back u_v / i_v only on request
        self.ranker.apply(self.ranker.init_weights)
        self.ranker.to(self.device)
        self.ranker_emb_size = ranker_args.emb_size
        self.restore_ranker()

    def restore_ranker(self):
        self.ranker.load_model(self._ranker_model_path)
        for p in self.ranker.parameters():
            p.requires_grad = False
        self.ranker.eval()

    def train(self, mode=True):
        super().train(mode)
        if getattr(self, 'ranker', None) is not None:
            self.ranker.eval()      # frozen: no dropout in the base ranker, whatever the head's mode
        return self

    def run_ranker(self, feed_dict):
        with torch.no_grad():
            out = self.ranker(utils.batch_to_gpu(feed_dict, self.device))
        if 'u_v' not in out or 'i_v' not in out:
            raise ValueError('{}Impression does not return u_v / i_v: it cannot serve as a base ranker'.format(self.ranker_name))
        return out

    def add_ranker_outputs(self, feed_dict, n_lists):
        """what the reference's collate_batch adds (:70-84), for both bases"""
        feed_dict['batch_size'] = n_lists
        out = self.run_ranker(feed_dict)
        dev = out['prediction'].device
        P, N = self.train_max_pos_item, self.train_max_neg_item
        pos_mask = torch.arange(P, device=dev)[None, :] < feed_dict['pos_num'].to(dev)[:, None]
        neg_mask = torch.arange(N, device=dev)[None, :] < feed_dict['neg_num'].to(dev)[:, None]
        all_mask = torch.cat([pos_mask, neg_mask], dim=1)
        feed_dict['padding_mask'] = ~all_mask
        feed_dict['scores'], feed_dict['position'] = rank_positions(out['prediction'], all_mask)
        feed_dict['u_v'], feed_dict['i_v'] = out['u_v'], out['i_v']
        return feed_dict

    class Dataset(ImpressionModel.Dataset):
        def collate_batch(self, feed_dicts: List[dict]) -> dict:
            return self.model.add_ranker_outputs(super().collate_batch(feed_dicts), len(feed_dicts))


class RerankSeqModel(RerankModel):
    reader = 'ImpressionSeqReader'
    runner = 'ImpressionRunner'
    extra_log_args = ['tuneranker']

    @staticmethod
    def parse_model_args(parser):
        parser.add_argument('--history_max', type=int, default=20, help='Maximum length of history.')
        parser.add_argument('--ranker_name', type=str, default='SASRec', help='Base ranker')
        parser.add_argument('--ranker_config_file', type=str, default='SASRec.yaml', help='Base ranker config file')
        parser.add_argument('--ranker_model_file', type=str, default='SASRec.pt', help='Base ranker model file')
        parser.add_argument('--tuneranker', type=int, default=0, help='if 1, continue to train ranker (not supported)')
        return ImpressionModel.parse_model_args(parser)

    def __init__(self, args, corpus):
        super().__init__(args, corpus)
        self.history_max = args.history_max

    class Dataset(ImpressionSeqModel.Dataset):
        def collate_batch(self, feed_dicts: List[dict]) -> dict:
            model = self.model
            feed_dict = model.add_ranker_outputs(super().collate_batch(feed_dicts), len(feed_dicts))
            ranker, his = model.ranker, feed_dict['history_items'].to(model.device)
            with torch.no_grad():
                if 'LightGCN' in model.ranker_name:
                    feed_dict['his_v'] = ranker.encoder.embedding_dict['item_emb'][his, :]
                else:
                    feed_dict['his_v'] = ranker.i_embeddings(his)
            return feed_dict

