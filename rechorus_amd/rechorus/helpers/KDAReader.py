"""KDAReader: KGReader + the frequency-domain initialisation of KDA's temporal kernels (mirror of helpers/KDAReader.py:15-106).

For the virtual relation (any two consecutive events of a user), every attribute relation (consecutive events of a user that share
the attribute's value) and every natural item relation (for each event, the most recent earlier event of the user whose item is a
head of the relation towards it) the positive time intervals are counted, normalised with `norm_time` (log2 of the interval in
units of --t_scalar, floored at 0), histogrammed in unit bins, scaled to a maximum of 1, and transformed with `dft`: `freq_x`
[n_relations, n_dft // 2 + 1] complex, the positive half of an n_dft-point DFT with the negative frequencies folded in (times 2).
The interval lists are cached in <dataset>/interval.pkl (--regenerate 1 recounts).  With --freq_rand 1 nothing is counted and
`freq_x` is left uninitialised, as in the reference (the model then keeps its random initialisation).

As in the reference, `n_dft` is widened to the smallest power of two above the largest bin count -- after `freq_x` was allocated
for the flag's value, so a corpus whose intervals span more than --n_dft bins fails at the assignment (:88-104), here with a
message that names the flag.
"""
import logging
import os
import pickle

import numpy as np
import pandas as pd

from helpers.KGReader import KGReader


class KDAReader(KGReader):
    @staticmethod
    def parse_data_args(parser):
        parser.add_argument('--t_scalar', type=int, default=60, help='Time interval scalar.')
        parser.add_argument('--n_dft', type=int, default=64, help='The point of DFT.')
        parser.add_argument('--freq_rand', type=int, default=0,
                            help='Whether randomly initialize parameters in frequency domain.')
        return KGReader.parse_data_args(parser)

    @staticmethod
    def dft(x, n_dft=-1) -> np.ndarray:
        if n_dft <= 0:
            n_dft = 2 ** (int(np.log2(len(x))) + 1)
        return 2 * np.fft.fft(x, n_dft)[: n_dft // 2 + 1]   # fold negative frequencies

    @staticmethod
    def norm_time(a, t_scalar) -> np.ndarray:
        return np.maximum(np.log2(np.array(a) / t_scalar + 1e-6), 0)

    def __init__(self, args):
        super().__init__(args)
        self.t_scalar, self.n_dft, self.freq_rand = args.t_scalar, args.n_dft, args.freq_rand
        self.regenerate = args.regenerate
        self.interval_file = os.path.join(self.prefix, self.dataset, 'interval.pkl')
        self.freq_x = np.empty((self.n_relations, self.n_dft // 2 + 1), dtype=complex)
        if not self.freq_rand:
            self._time_interval_cnt()
            self._cal_freq_x()

    def _time_interval_cnt(self):
        """interval_dict: 'virtual' and every relation name -> the list of positive time intervals (:53-85)"""
        if os.path.exists(self.interval_file) and not self.regenerate:
            with open(self.interval_file, 'rb') as f:
                self.interval_dict = pickle.load(f)
            return
        logging.info('Counting time intervals of relational neighbours...')
        self.interval_dict = {'virtual': []}
        for relation in self.relations:
            self.interval_dict[relation] = []
        merged = pd.merge(self.all_df, self.item_meta_df, how='left', on='item_id')
        for _, user_df in merged.groupby('user_id'):
            times, iids = user_df['time'].values, user_df['item_id'].values
            gaps = times[1:] - times[:-1]
            self.interval_dict['virtual'].extend(gaps[gaps > 0].tolist())
            for attr in self.attr_relations:
                for _, same in user_df.groupby(attr):
                    t = same['time'].values
                    gaps = t[1:] - t[:-1]
                    self.interval_dict[attr].extend(gaps[gaps > 0].tolist())
            for k, relation in enumerate(self.item_relations):
                for target in range(len(iids) - 1, 0, -1):          # tail items back to front
                    for source in range(target - 1, -1, -1):        # the most recent related head
                        gap = times[target] - times[source]
                        if gap > 0 and (iids[source], k + 1, iids[target]) in self.triplet_set:
                            self.interval_dict[relation].append(gap)
                            break
        with open(self.interval_file, 'wb') as f:
            pickle.dump(self.interval_dict, f)

    def _cal_freq_x(self):
        distributions = []
        for col in ['virtual'] + self.relations:
            intervals = self.norm_time(self.interval_dict[col], self.t_scalar)
            bin_num = int(max(intervals)) + 1
            ns = np.zeros(bin_num)
            np.add.at(ns, intervals.astype(int), 1)
            distributions.append(ns / max(ns))
            self.n_dft = max(self.n_dft, 2 ** (int(np.log2(bin_num) + 1)))
        if self.freq_x.shape[1] != self.n_dft // 2 + 1:
            raise ValueError('KDAReader: the time intervals span more bins than --n_dft {} covers; pass --n_dft {}'.format(
                (self.freq_x.shape[1] - 1) * 2, self.n_dft))
        for i, dist in enumerate(distributions):
            self.freq_x[i] = self.dft(dist, self.n_dft)
        del self.interval_dict
