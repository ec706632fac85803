"""ContextSeqReader: ContextReader + per-user interaction history WITH the situation context of every past interaction
(counterpart of the reference's helpers/ContextSeqReader.py:13-43; same corpus attributes).

`user_his[uid] = [(item, time, situation values), ...]` in global (time, user) order, the situation values as one array in
`situation_feature_names` order (empty without --include_situation_features), and a `position` column in every data_df: the
index of the interaction inside its user's history, i.e. how many earlier interactions the user has.  The history-aware context
Datasets (models/BaseContextModel.py: ContextSeqModel, ContextSeqCTRModel) cut `user_his[uid][:position]`."""
import logging

import pandas as pd

from helpers.ContextReader import ContextReader


class ContextSeqReader(ContextReader):
    def __init__(self, args):
        super().__init__(args)
        self._append_his_info()

    def _append_his_info(self):
        logging.info('Appending history info with history context...')
        cols = ['user_id', 'item_id', 'time'] + self.situation_feature_names
        ordered = pd.concat([self.data_df[phase][cols] for phase in ('train', 'dev', 'test')])
        ordered = ordered.sort_values(by=['time', 'user_id'], kind='mergesort')
        ordered['position'] = ordered.groupby('user_id').cumcount()
        situations = ordered[self.situation_feature_names].to_numpy()
        self.user_his = {}
        for row, (uid, iid, t) in enumerate(zip(ordered['user_id'], ordered['item_id'], ordered['time'])):
            self.user_his.setdefault(uid, []).append((iid, t, situations[row]))
        keys = ordered[['user_id', 'item_id', 'time', 'position']]
        for phase in ('train', 'dev', 'test'):
            self.data_df[phase] = pd.merge(left=self.data_df[phase], right=keys, how='left', on=['user_id', 'item_id', 'time'])
