"""DownscalingWorkflow: a chain of Downscaling tasks, one per level, and WriteDownscalingMetadata
(cluster_tools/downscaling/downscaling_workflow.py:33-347; parameters, config keys, scale keys,
task prefixes and the paintera attributes unchanged).  Every level `s<k + 1>` is written next to
the input, `s<scale_offset>` is a symbolic link to the input dataset, and the group gets
`multiScale`, `resolution`, `offset` and the copied `maxId`, every level its `downsamplingFactors`
against the original resolution, reversed to XYZ.

`metadata_format='bdv'` needs HDF5 containers, which cluster_tools_amd.io does not have:
`validate_format` raises NotImplementedError for it.  PainteraToBdvWorkflow (:352-465, a copy into
HDF5) and the Upscaling tasks of the reference package are not built."""
import os
from datetime import datetime

from cluster_tools_amd import luigi_compat as luigi
from cluster_tools_amd.cluster_tasks import WorkflowBase
from cluster_tools_amd.utils.volume_utils import file_reader
from cluster_tools_amd.downscaling import downscaling as downscale_tasks


def _accumulate(effective_scale, scale_factor):
    """The scale against the original resolution after one more level."""
    if isinstance(scale_factor, int):
        return [eff * scale_factor for eff in effective_scale]
    return [eff * sf for sf, eff in zip(scale_factor, effective_scale)]


class WriteDownscalingMetadata(luigi.Task):
    tmp_folder = luigi.Parameter()
    output_path = luigi.Parameter()
    scale_factors = luigi.ListParameter()
    dependency = luigi.TaskParameter()
    metadata_format = luigi.Parameter(default='paintera')
    metadata_dict = luigi.DictParameter(default={})
    output_key_prefix = luigi.Parameter(default='')
    scale_offset = luigi.IntParameter(default=0)

    def requires(self):
        return self.dependency

    def _write_log(self, msg):
        with open(self.output().path, 'a') as f:
            f.write('%s: %s\n' % (str(datetime.now()), msg))

    def _paintera_metadata(self):
        effective_scale = [1, 1, 1]
        with file_reader(self.output_path) as f:
            for scale, scale_factor in enumerate(self.scale_factors):
                # 's0' is the original resolution
                key = os.path.join(self.output_key_prefix, 's%i' % (scale + self.scale_offset + 1))
                effective_scale = _accumulate(effective_scale, scale_factor)
                f[key].attrs['downsamplingFactors'] = effective_scale[::-1]
            group = f[self.output_key_prefix]
            group.attrs['multiScale'] = True
            group.attrs['resolution'] = list(self.metadata_dict.get('resolution', 3 * [1.]))[::-1]
            group.attrs['offset'] = list(self.metadata_dict.get('offsets', 3 * [0.]))[::-1]
            attrs0 = f[os.path.join(self.output_key_prefix, 's%i' % self.scale_offset)].attrs
            if 'maxId' in attrs0:
                group.attrs['maxId'] = attrs0['maxId']

    def run(self):
        if self.metadata_format == 'paintera':
            self._paintera_metadata()
        elif self.metadata_format == 'bdv':
            raise NotImplementedError("bdv metadata needs an HDF5 container, which cluster_tools_amd.io does not have")
        else:
            raise RuntimeError("Invalid metadata format %s" % self.metadata_format)
        self._write_log('write metadata successfull')

    def output(self):
        return luigi.LocalTarget(os.path.join(self.tmp_folder, 'write_downscaling_metadata.log'))


class DownscalingWorkflow(WorkflowBase):
    input_path = luigi.Parameter()
    input_key = luigi.Parameter()
    scale_factors = luigi.ListParameter()
    halos = luigi.ListParameter()
    metadata_format = luigi.Parameter(default='paintera')
    metadata_dict = luigi.DictParameter(default={})
    output_key_prefix = luigi.Parameter(default='')
    skip_existing_levels = luigi.BoolParameter(default=False)
    scale_offset = luigi.IntParameter(default=0)

    @staticmethod
    def validate_scale_factors(scale_factors):
        assert all(isinstance(sf, (int, list, tuple)) for sf in scale_factors)
        assert all(len(sf) == 3 for sf in scale_factors if isinstance(sf, (tuple, list)))

    @staticmethod
    def validate_halos(halos, n_scales):
        assert len(halos) == n_scales, "%i, %i" % (len(halos), n_scales)
        halos = [[] if halo is None else list(halo) for halo in halos]
        assert all(len(halo) == 3 for halo in halos if halo)
        return halos

    def validate_format(self):
        assert self.metadata_format in ('paintera', 'bdv'), "Invalid format %s" % self.metadata_format
        if self.metadata_format == 'bdv':
            raise NotImplementedError("DownscalingWorkflow: metadata_format 'bdv' needs an HDF5 container, which "
                                      "cluster_tools_amd.io does not have; use metadata_format 'paintera' (n5)")
        assert self.output_key_prefix != '', "Need output_key_prefix for paintera data format"

    def get_scale_key(self, scale):
        # 's0' is the original resolution
        return os.path.join(self.output_key_prefix, 's%i' % (scale + 1,))

    def _link_scale_zero(self, key):
        """`key` becomes a symbolic link to the input dataset, unless it exists."""
        with file_reader(self.input_path) as f:
            if key in f:
                return
        src = os.path.abspath(os.path.realpath(os.path.join(self.input_path, self.input_key)))
        dst = os.path.abspath(os.path.realpath(os.path.join(self.input_path, key)))
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        os.symlink(src, dst)

    def _have_scale(self, scale):
        with file_reader(self.input_path) as f:
            return self.get_scale_key(scale) in f

    def requires(self):
        self.validate_scale_factors(self.scale_factors)
        halos = self.validate_halos(self.halos, len(self.scale_factors))
        self.validate_format()
        ds_task = getattr(downscale_tasks, self._get_task_name('Downscaling'))

        in_key = self.get_scale_key(self.scale_offset - 1)
        self._link_scale_zero(in_key)
        dep = self.dependency
        effective_scale = [1, 1, 1]
        for level, scale_factor in enumerate(self.scale_factors):
            scale = level + self.scale_offset
            out_key = self.get_scale_key(scale)
            effective_scale = _accumulate(effective_scale, scale_factor)
            if self.skip_existing_levels and self._have_scale(scale):
                in_key = out_key
                continue
            dep = ds_task(tmp_folder=self.tmp_folder, max_jobs=self.max_jobs, config_dir=self.config_dir,
                          input_path=self.input_path, input_key=in_key, output_path=self.input_path,
                          output_key=out_key, scale_factor=scale_factor, scale_prefix='s%i' % (scale + 1,),
                          effective_scale_factor=effective_scale, halo=halos[level], dependency=dep)
            in_key = out_key

        return WriteDownscalingMetadata(tmp_folder=self.tmp_folder, output_path=self.input_path,
                                        output_key_prefix=self.output_key_prefix,
                                        metadata_format=self.metadata_format, metadata_dict=self.metadata_dict,
                                        scale_factors=self.scale_factors, scale_offset=self.scale_offset,
                                        dependency=dep)

    @staticmethod
    def get_config():
        configs = WorkflowBase.get_config()
        configs.update({'downscaling': downscale_tasks.DownscalingLocal.default_task_config()})
        return configs
