!=======================================================================
! compute_ponds and increment_age on the GPU for a caller of the reference's driver.
!
! A module of its own name, next to ice_coupling_gpu.  It offers
!   step_ponds_gpu    the two calls of step_therm1's category loop that cice_step_therm1 leaves out
!                     (drivers/cice4/CICE_RunMod.F90:449-454 increment_age, :550-559 compute_ponds) as ONE cice_step_ponds
!                     (include/cice4_amd.h) on the module arrays of ice_state and ice_flux, for all categories and blocks.
! The call goes BEHIND cice_step_therm1 and in front of cice_step_therm2_itd: thermo_vertical neither reads nor writes the
! age tracer, and aicen is intent(in) there, so the list is the same before and after.
! The reference's conditions stay the reference's: ponds run under `tr_pond .and. trim(shortwave) == 'dEdd'`, the age under
! tr_iage; with neither the routine returns at once.
! cice_thermo_init and cice_pond_init are made on the first call, which is after the namelist.
!=======================================================================
      module ice_pond_gpu

      use ice_kinds_mod
      use ice_domain_size, only: ncat, nilyr, nslyr, max_ntrcr
      use iso_c_binding
      use cice4_amd_c

      implicit none
      save
      private
      public :: step_ponds_gpu

      logical, private :: pond_ready = .false., batch_ready = .false.

      contains

!=======================================================================
      subroutine pond_ensure
      use ice_state, only: nt_Tsfc, nt_iage, nt_volpn
      use ice_age, only: tr_iage
      use ice_meltpond, only: tr_pond
      use ice_therm_vertical, only: heat_capacity, calc_Tsfc, conduct, ustar_min
      use ice_blocks, only: nx_block, ny_block
      use ice_domain, only: nblocks
      type (cice_thermo_config) :: tcfg
      real (kind=dbl_kind) :: sal(nilyr+1), tml(nilyr+1)
      if (.not. pond_ready) then
         call cice_gpu_ensure()
         call cice_gpu_check(cice_check_sizes(cice_gpu_ctx, ncat, nilyr, nslyr, max_ntrcr), 'ice_pond_gpu')
         tcfg%heat_capacity = merge(1, 0, heat_capacity)
         tcfg%calc_Tsfc = merge(1, 0, calc_Tsfc)
         tcfg%conduct = merge(0, 1, trim(conduct) == 'MU71')
         tcfg%ustar_min = ustar_min
         tcfg%tr_iage = merge(1, 0, tr_iage)
         tcfg%nt_Tsfc = nt_Tsfc
         tcfg%nt_iage = nt_iage
         call cice_gpu_check(cice_thermo_init(cice_gpu_ctx, tcfg, sal, tml), 'cice_thermo_init')
         call cice_gpu_check(cice_pond_init(cice_gpu_ctx, merge(nt_volpn, 0, tr_pond)), 'cice_pond_init')
         pond_ready = .true.
      endif
      if (.not. batch_ready) then
         call cice_gpu_check(cice_thermo_batch_alloc(cice_gpu_ctx, nx_block, ny_block, nblocks), 'ice_pond_gpu')
         batch_ready = .true.
      endif
      end subroutine pond_ensure

!=======================================================================
! state_resident: aicen, vicen, vsnon, the surface temperature and the per-category meltt, melts are what cice_step_therm1
!                 left on the device in this step (default .true.: the driver keeps melttn, meltsn in locals of step_therm1)
! melttn, meltsn: (nx_block,ny_block,ncat,nblocks), needed with state_resident = .false. and ponds
      subroutine step_ponds_gpu (dt, state_resident, melttn, meltsn)
      use ice_state, only: aicen, vicen, vsnon, trcrn, apondn, hpondn
      use ice_flux, only: frain
      use ice_age, only: tr_iage
      use ice_meltpond, only: tr_pond
      use ice_shortwave, only: shortwave
      use ice_exit, only: abort_ice
      real (kind=dbl_kind), intent(in) :: dt
      logical (kind=log_kind), intent(in), optional :: state_resident
      real (kind=dbl_kind), intent(in), optional, target :: melttn(*), meltsn(*)
      type (cice_pond_fields) :: f
      logical :: ponds

      ponds = tr_pond .and. trim(shortwave) == 'dEdd'
      if (.not. ponds .and. .not. tr_iage) return
      call pond_ensure
      f%ncat = ncat
      f%state_resident = 1
      if (present(state_resident)) f%state_resident = merge(1, 0, state_resident)
      f%ponds = merge(1, 0, ponds)
      f%age = merge(1, 0, tr_iage)
      f%frain = addr_r8(frain)
      f%trcrn = addr_r8(trcrn)
      f%apondn = addr_r8(apondn); f%hpondn = addr_r8(hpondn)
      f%aicen = addr_r8(aicen); f%vicen = addr_r8(vicen); f%vsnon = addr_r8(vsnon)
      f%melttn = c_null_ptr; f%meltsn = c_null_ptr
      if (present(melttn)) f%melttn = c_loc(melttn)
      if (present(meltsn)) f%meltsn = c_loc(meltsn)
      if (f%state_resident == 0 .and. ponds .and. .not. (present(melttn) .and. present(meltsn))) &
         call abort_ice ('step_ponds_gpu: state_resident = .false. needs melttn and meltsn')
      call cice_gpu_check(cice_step_ponds(cice_gpu_ctx, dt, f), 'step_ponds_gpu')
      end subroutine step_ponds_gpu

      end module ice_pond_gpu
