"""KGReader: SeqReader + the item knowledge graph of item_meta.csv (mirror of helpers/KGReader.py:15-73).

item_meta.csv (the reader's separator; list columns are python literals) contributes two kinds of relation:
  item-item   every column whose name starts with 'r_' holds, per item, a list of tail items; column number k (in column order)
              is relation k + 1 -- relation 0 is reserved for "the item itself" -- and yields one triplet (head, k + 1, tail) per
              list entry;
  attribute   with --include_attr 1, every column starting with 'i_': value val != 0 of attribute number k becomes the entity
              val + n_items + sum(attr_max[:k]) (attr_max[k] = the column's maximum + 1), relation len(item_relations) + k + 1;
              share_attr_dict[entity] lists the items that carry the value.
Attributes left behind: item_meta_df, triplet_set, item_relations, attr_relations, relations, relation_df (head, relation, tail in
emission order), n_relations = len(relations) + 1, n_entities = the largest head or tail + 1.
"""
import logging
import os

import numpy as np
import pandas as pd

from helpers.SeqReader import SeqReader
from utils import utils


class KGReader(SeqReader):
    @staticmethod
    def parse_data_args(parser):
        parser.add_argument('--include_attr', type=int, default=0, help='Whether include attribute-based relations.')
        return SeqReader.parse_data_args(parser)

    def __init__(self, args):
        super().__init__(args)
        self.include_attr = args.include_attr
        meta = pd.read_csv(os.path.join(self.prefix, self.dataset, 'item_meta.csv'), sep=self.sep)
        self.item_meta_df = utils.eval_list_columns(meta)
        self._construct_kg()

    def _construct_kg(self):
        logging.info('Constructing relation triplets...')
        meta = self.item_meta_df
        items = meta['item_id'].tolist()
        triplets = []   # (head, relation, tail) in emission order: item by item, relation by relation, tail by tail
        self.item_relations = [c for c in meta.columns if c.startswith('r_')]
        tails_of = [meta[c].tolist() for c in self.item_relations]
        for row, head in enumerate(items):
            for k, tails in enumerate(tails_of):
                triplets.extend((head, k + 1, tail) for tail in tails[row])
        logging.info('Item-item relations:' + str(self.item_relations))

        self.attr_relations = []
        if self.include_attr:
            self.attr_relations = [c for c in meta.columns if c.startswith('i_')]
            self.attr_max, self.share_attr_dict = [], {}
            for k, attr in enumerate(self.attr_relations):
                base = self.n_items + np.sum(self.attr_max)   # the first entity id of this attribute
                relation = len(self.item_relations) + k + 1
                values = meta[attr].tolist()
                triplets.extend((item, relation, int(val + base)) for item, val in zip(items, values) if val != 0)
                for val, grp in meta.groupby(attr):
                    self.share_attr_dict[int(val + base)] = grp['item_id'].tolist()
                self.attr_max.append(meta[attr].max() + 1)
            logging.info('Attribute-based relations:' + str(self.attr_relations))

        self.triplet_set = set(triplets)
        self.relations = self.item_relations + self.attr_relations
        self.relation_df = pd.DataFrame(triplets, columns=['head', 'relation', 'tail'])
        self.n_relations = len(self.relations) + 1
        self.n_entities = pd.concat((self.relation_df['head'], self.relation_df['tail'])).max() + 1
        logging.info('"# relation": {}, "# triplet": {}'.format(self.n_relations, len(self.relation_df)))
