"""Context-aware model bases (mirror of the reference's models/BaseContextModel.py:16-89):
ContextModel (top-k ranking with BPR or BCE loss) and ContextCTRModel (labelled click data).
Both add the corpus' user / item / situation features to every feed dict; the model sees them
as extra int (or float) tensors keyed by feature name next to 'user_id' / 'item_id'.

ContextSeqModel / ContextSeqCTRModel (reference :89-166, reader helpers.ContextSeqReader) add the user's history to the
feed: `history_item_id`, `history_<item feature>`, with --add_historical_situations 1 also `history_<situation feature>`, and
`lengths`; histories are cut to the last --history_max interactions and instances without history are dropped.
"""
import numpy as np
import torch

from models.BaseModel import GeneralModel, CTRModel, SequentialModel
from rechorus_amd import nn as hnn


def get_context_feature(feed_dict, index, corpus, data):
    """user features by user id, situation features by row, item features per candidate"""
    for c in corpus.user_feature_names:
        feed_dict[c] = corpus.user_features[feed_dict['user_id']][c]
    for c in corpus.situation_feature_names:
        feed_dict[c] = data[c][index]
    items = feed_dict['item_id']
    for c in corpus.item_feature_names:
        if isinstance(items, (int, np.integer)):
            feed_dict[c] = corpus.item_features[items][c]
        else:
            feed_dict[c] = np.array([corpus.item_features[i][c] for i in items])
    return feed_dict


def _feature_list(corpus):
    return (corpus.user_feature_names + corpus.item_feature_names + corpus.situation_feature_names
            + ['user_id', 'item_id'])


class ContextModel(GeneralModel):
    reader = 'ContextReader'

    @staticmethod
    def parse_model_args(parser):
        parser.add_argument('--loss_n', type=str, default='BPR', help='Type of loss functions.')
        return GeneralModel.parse_model_args(parser)

    def __init__(self, args, corpus):
        super().__init__(args, corpus)
        self.loss_n = args.loss_n
        self.context_features = _feature_list(corpus)
        self.feature_max = corpus.feature_max

    def loss(self, out_dict: dict):
        """BPR (the HIP loss kernel of GeneralModel) or point-wise BCE over pos + negs (:49-63)"""
        if self.loss_n == 'BPR':
            return super().loss(out_dict)
        if self.loss_n == 'BCE':  # one HIP kernel, closed-form backward
            if not out_dict['prediction'].is_cuda:
                raise RuntimeError('ContextModel.loss: the HIP engine needs CUDA tensors (no CPU path)')
            return hnn.bce_ranking_loss(out_dict['prediction'])
        raise ValueError('Undefined loss function: {}'.format(self.loss_n))

    class Dataset(GeneralModel.Dataset):
        def _get_feed_dict(self, index):
            feed = super()._get_feed_dict(index)
            return get_context_feature(feed, index, self.corpus, self.data)


class ContextCTRModel(CTRModel):
    reader = 'ContextReader'

    def __init__(self, args, corpus):
        super().__init__(args, corpus)
        self.context_features = _feature_list(corpus)
        self.feature_max = corpus.feature_max

    class Dataset(CTRModel.Dataset):
        def _get_feed_dict(self, index):
            feed = super()._get_feed_dict(index)
            return get_context_feature(feed, index, self.corpus, self.data)


def _seq_flags(parser):
    parser.add_argument('--history_max', type=int, default=20, help='Maximum length of history.')
    parser.add_argument('--add_historical_situations', type=int, default=0,
                        help='Whether to add historical situation context as sequence.')
    return parser


def _history_context(feed, model, corpus, user_seq):
    """the history's item features per position, its situation features where the model asks for them, and the reference's key
    `history_item_id` for the item ids (:117-123, :159-165)"""
    items = feed.pop('history_items')
    for c in corpus.item_feature_names:
        feed['history_' + c] = np.array([corpus.item_features[i][c] for i in items])
    if model.add_historical_situations:
        for k, c in enumerate(corpus.situation_feature_names):
            feed['history_' + c] = np.array([inter[-1][k] for inter in user_seq])
    feed['history_item_id'] = items
    return feed


def _cut_history(model, corpus, user_id, position):
    seq = corpus.user_his[user_id][:position]
    return seq[-model.history_max:] if model.history_max > 0 else seq


class ContextSeqModel(ContextModel):
    reader = 'ContextSeqReader'

    @staticmethod
    def parse_model_args(parser):
        return ContextModel.parse_model_args(_seq_flags(parser))

    def __init__(self, args, corpus):
        super().__init__(args, corpus)
        self.history_max = args.history_max
        self.add_historical_situations = args.add_historical_situations

    class Dataset(SequentialModel.Dataset):
        def _get_feed_dict(self, index):
            feed = super()._get_feed_dict(index)      # user, candidates, history_items / history_times / lengths
            seq = _cut_history(self.model, self.corpus, feed['user_id'], self.data['position'][index])
            feed = get_context_feature(feed, index, self.corpus, self.data)
            return _history_context(feed, self.model, self.corpus, seq)


class ContextSeqCTRModel(ContextCTRModel):
    reader = 'ContextSeqReader'

    @staticmethod
    def parse_model_args(parser):
        return ContextCTRModel.parse_model_args(_seq_flags(parser))

    def __init__(self, args, corpus):
        super().__init__(args, corpus)
        self.history_max = args.history_max
        self.add_historical_situations = args.add_historical_situations

    class Dataset(ContextCTRModel.Dataset):
        def __init__(self, model, corpus, phase):
            super().__init__(model, corpus, phase)
            keep = np.array(self.data['position']) > 0      # the history must not be empty
            for col in self.data:
                self.data[col] = np.array(self.data[col])[keep]

        def _get_feed_dict(self, index):
            feed = super()._get_feed_dict(index)
            seq = _cut_history(self.model, self.corpus, feed['user_id'], self.data['position'][index])
            feed['history_items'] = np.array([x[0] for x in seq])
            feed['history_times'] = np.array([x[1] for x in seq])
            feed['lengths'] = len(seq)
            return _history_context(feed, self.model, self.corpus, seq)
